"""What every job script takes from utils/function_utils.py: the device of the job, the read-ahead
loop (exactly one read ahead of the body, on one thread), the config preamble and the entry point.
CPU only; every wait is on an event with a timeout, so a missing overlap fails instead of hanging."""
import json
import sys
import threading

import pytest

import cluster_tools_amd.utils.function_utils as fu

WAIT = 5.


class RecordingRead:
    """read(i) -> 10 * i; an event per item for "has started" and "has finished"."""

    def __init__(self, n, fail_at=None):
        self.started = [threading.Event() for _ in range(n)]
        self.finished = [threading.Event() for _ in range(n)]
        self.order = []
        self.fail_at = fail_at

    def __call__(self, i):
        self.started[i].set()
        self.order.append(i)
        try:
            if i == self.fail_at:
                raise ValueError("read of item %i" % i)
            return 10 * i
        finally:
            self.finished[i].set()


def test_pairs_in_order_with_results():
    read = RecordingRead(5)
    seen = []
    with fu.read_ahead(read, list(range(5))) as ahead:
        for item, fut in ahead:
            seen.append((item, fut.result(WAIT)))
    assert seen == [(i, 10 * i) for i in range(5)]
    assert read.order == list(range(5))


def test_items_need_not_be_ints():
    batches = [[0, 1], [2, 3], [4]]
    with fu.read_ahead(sum, batches) as ahead:
        assert [(item, fut.result(WAIT)) for item, fut in ahead] == [([0, 1], 1), ([2, 3], 5), ([4], 4)]


@pytest.mark.parametrize('items', [[], range(0)])
def test_empty_input(items):
    read = RecordingRead(1)
    with fu.read_ahead(read, items) as ahead:
        assert list(ahead) == []
    assert read.order == []


def test_first_read_starts_at_entry():
    read = RecordingRead(3)
    with fu.read_ahead(read, [0, 1, 2]) as ahead:
        # nothing has been taken from `ahead` yet
        assert read.started[0].wait(WAIT)
        assert read.finished[0].wait(WAIT)
        assert not read.started[1].is_set()
        assert [item for item, _ in ahead] == [0, 1, 2]


def test_exactly_one_read_ahead_of_the_body():
    n = 5
    read = RecordingRead(n)
    with fu.read_ahead(read, list(range(n))) as ahead:
        for k, fut in ahead:
            assert fut.result(WAIT) == 10 * k
            if k + 1 < n:
                # the overlap: the next read runs while this body does
                assert read.started[k + 1].wait(WAIT), "read %i did not start during the body of %i" % (k + 1, k)
                assert read.finished[k + 1].wait(WAIT)
            if k + 2 < n:
                # ... and the reader is idle after it: nothing later was submitted.  (Against a loop
                # that ran further ahead this check races with the reader thread, which starts
                # read k + 2 only after read k + 1 has ended; test_submits_exactly_one_ahead below
                # sees the submissions themselves and does not.)
                assert not read.started[k + 2].is_set(), "read %i started during the body of %i" % (k + 2, k)
    assert read.order == list(range(n))


def test_submits_exactly_one_ahead(monkeypatch):
    """The same contract seen at submit(), on the caller's thread: no race with the reader."""
    submitted = []

    class Recording(fu.futures.ThreadPoolExecutor):
        def submit(self, fn, item):
            submitted.append(item)
            return super().submit(fn, item)

    monkeypatch.setattr(fu.futures, 'ThreadPoolExecutor', Recording)
    items = list('abcde')
    with fu.read_ahead(str.upper, items) as ahead:
        assert submitted == ['a']
        for k, (item, fut) in enumerate(ahead):
            assert submitted == items[:k + 2]
            assert fut.result(WAIT) == item.upper()
            assert submitted == items[:k + 2]
    assert submitted == items


def test_read_error_surfaces_at_its_item():
    read = RecordingRead(5, fail_at=3)
    results = {}
    with fu.read_ahead(read, list(range(5))) as ahead:
        for item, fut in ahead:
            if item == 3:
                with pytest.raises(ValueError, match="read of item 3"):
                    fut.result(WAIT)
            else:
                results[item] = fut.result(WAIT)
    # not earlier, not at exit, and the reader went on
    assert results == {0: 0, 1: 10, 2: 20, 4: 40}


def test_read_error_leaves_the_context_as_a_job_would():
    read = RecordingRead(5, fail_at=3)
    done = []
    with pytest.raises(ValueError, match="read of item 3"):
        with fu.read_ahead(read, list(range(5))) as ahead:
            for item, fut in ahead:
                fut.result(WAIT)
                done.append(item)
    assert done == [0, 1, 2]
    # the one read that was ahead has run to its end before the context is left: nothing runs on
    assert read.order == [0, 1, 2, 3, 4] and read.finished[4].is_set()


def test_device(monkeypatch):
    monkeypatch.setenv('CTWS_DEVICE', '2')
    monkeypatch.setenv('LOCAL_RANK', '5')
    assert fu.device() == 2
    monkeypatch.delenv('CTWS_DEVICE')
    assert fu.device() == 5
    monkeypatch.delenv('LOCAL_RANK')
    assert fu.device() == 0


def test_no_job_script_chooses_its_device_itself():
    """Every job takes fu.device(): a copy of the rule in a script is how two jobs came to ignore
    LOCAL_RANK.  (watershed.py only asks whether CTWS_DEVICE is set, to choose a backend.)"""
    import glob
    import os
    import re
    package = os.path.dirname(os.path.dirname(os.path.abspath(fu.__file__)))
    scripts = sorted(glob.glob(os.path.join(package, '*', '*.py')))
    assert len(scripts) > 30
    own_rule = re.compile(r"def _device\(|environ(\.get\(|\[)\s*['\"](CTWS_DEVICE|LOCAL_RANK)['\"]")
    offenders = [os.path.relpath(p, package) for p in scripts
                 if os.path.abspath(p) != os.path.abspath(fu.__file__) and own_rule.search(open(p).read())]
    assert offenders == []


def test_job_id_from_path():
    assert fu.job_id_from_path('/tmp/ws/block_morphology_12.config') == 12
    assert fu.job_id_from_path('/tmp/ws/block_node_labels_seg_3.config') == 3
    assert fu.job_id_from_path('write_7.config') == 7


def test_run_job(tmp_path, monkeypatch):
    path = tmp_path / 'block_node_labels_seg_3.config'
    path.write_text('{}')
    calls = []
    monkeypatch.setattr(sys, 'argv', ['job.py', str(path)])
    fu.run_job(lambda job_id, config_path: calls.append((job_id, config_path)))
    assert calls == [(3, str(path))]


def test_run_job_missing_file(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(sys, 'argv', ['job.py', str(tmp_path / 'write_0.config')])
    with pytest.raises(AssertionError):
        fu.run_job(lambda job_id, config_path: calls.append(job_id))
    assert calls == []


def test_load_config(tmp_path, capsys):
    path = tmp_path / 'write_4.config'
    config = {'block_list': [1, 2, 3], 'input_path': 'a.n5', 'ignore_label': None}
    path.write_text(json.dumps(config))
    assert fu.load_config(4, str(path)) == config
    lines = capsys.readouterr().out.splitlines()
    assert [line.split(': ', 1)[1] for line in lines] == ["start processing job 4", "reading config from %s" % path]


def test_chunk_id():
    from cluster_tools_amd.utils.blocking import Blocking
    blocking = Blocking([0, 0, 0], [20, 30, 40], [10, 10, 16])
    for block_id in range(blocking.numberOfBlocks):
        block = blocking.getBlock(block_id)
        cid = fu.chunk_id(block, blocking)
        assert all(isinstance(c, int) for c in cid)
        assert [c * s for c, s in zip(cid, [10, 10, 16])] == [int(b) for b in block.begin]
