"""CPU tests of the SizeFilterWorkflow task surface (cluster_tools/postprocess/
postprocess_workflow.py:24-112, size_filter_blocks.py, background_size_filter.py,
filling_size_filter.py): the size_filter_blocks job on hand-made temp files, task and workflow
parameters, config keys and the task graph of both variants.  No GPU call is made."""
import json
import os

import numpy as np
import pytest

from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.postprocess import SizeFilterWorkflow
from cluster_tools_amd.postprocess import size_filter_blocks as sfb
from cluster_tools_amd.postprocess import background_size_filter as bg
from cluster_tools_amd.postprocess import filling_size_filter as filling


def _run_job(tmp_path, tables, threshold):
    for j, (u, c) in enumerate(tables):
        np.save(str(tmp_path / ('find_uniques_job_%i.npy' % j)), np.asarray(u, dtype='uint64'))
        np.save(str(tmp_path / ('counts_job_%i.npy' % j)), np.asarray(c, dtype='uint64'))
    cfg = tmp_path / 'size_filter_blocks_job_0.config'
    cfg.write_text(json.dumps({'tmp_folder': str(tmp_path), 'n_jobs': len(tables), 'size_threshold': threshold}))
    sfb.size_filter_blocks(0, str(cfg))
    return np.load(str(tmp_path / 'discard_ids.npy'))


def test_size_filter_blocks_job_merges_counts(tmp_path, capsys):
    big = 2 ** 40
    tables = [([0, 3, 7, big + 1, big + 5], [4, 10, 2, 6, 100]),
              ([3, 7, 9, big + 1], [5, 3, 50, 6]),
              ([0, big + 9], [3, 1])]
    discard = _run_job(tmp_path, tables, 10)
    # 0: 7 (background below the threshold is discarded too), 3: 15, 7: 5, 9: 50,
    # big + 1: 12, big + 5: 100, big + 9: 1
    assert discard.dtype == np.uint64
    np.testing.assert_array_equal(discard, np.array([0, 7, big + 9], dtype=np.uint64))
    out = capsys.readouterr().out
    assert 'applying size filter 10' in out and 'discarding 3 / 7 ids' in out
    assert 'saving results to %s' % os.path.join(str(tmp_path), 'discard_ids.npy') in out
    assert out.rstrip().endswith('processed job 0')


def test_size_filter_blocks_job_matches_numpy(tmp_path):
    rng = np.random.default_rng(0)
    vol = rng.integers(0, 300, size=40000).astype(np.uint64) * np.uint64(2 ** 33 // 7)
    parts = np.array_split(vol, 3)
    tables = [np.unique(p, return_counts=True) for p in parts]
    ids, counts = np.unique(vol, return_counts=True)
    np.testing.assert_array_equal(_run_job(tmp_path, tables, 130), ids[counts < 130])
    u, c = sfb.merge_counts([t[0] for t in tables], [t[1] for t in tables])
    np.testing.assert_array_equal(u, ids)
    np.testing.assert_array_equal(c, counts.astype(np.uint64))


def test_nothing_below_the_threshold_gives_an_empty_list(tmp_path):
    discard = _run_job(tmp_path, [([1, 2], [50, 60])], 10)
    assert discard.dtype == np.uint64 and len(discard) == 0


def _names(cls):
    return [n for n, _ in cls.get_params()]


def test_task_parameters_and_names():
    common = ['tmp_folder', 'max_jobs', 'config_dir']
    assert sfb.SizeFilterBlocksLocal.task_name == 'size_filter_blocks'
    assert bg.BackgroundSizeFilterLocal.task_name == 'background_size_filter'
    assert filling.FillingSizeFilterLocal.task_name == 'filling_size_filter'
    assert sorted(_names(sfb.SizeFilterBlocksLocal)) == sorted(
        common + ['input_path', 'input_key', 'size_threshold', 'dependency'])
    assert sorted(_names(bg.BackgroundSizeFilterLocal)) == sorted(
        common + ['input_path', 'input_key', 'output_path', 'output_key', 'dependency'])
    assert sorted(_names(filling.FillingSizeFilterLocal)) == sorted(
        common + ['input_path', 'input_key', 'hmap_path', 'hmap_key', 'output_path', 'output_key', 'dependency'])
    assert sfb.SizeFilterBlocksLocal.allow_retry is False
    for mod, base in ((sfb, 'SizeFilterBlocks'), (bg, 'BackgroundSizeFilter'), (filling, 'FillingSizeFilter')):
        for target in ('Local', 'Slurm', 'LSF'):
            assert hasattr(mod, base + target)
    assert sorted(_names(SizeFilterWorkflow)) == sorted(
        common + ['target', 'dependency', 'input_path', 'input_key', 'output_path', 'output_key', 'size_threshold',
                  'hmap_path', 'hmap_key', 'relabel'])


def test_get_config_keys():
    cfg = SizeFilterWorkflow.get_config()
    assert sorted(cfg) == ['background_size_filter', 'filling_size_filter', 'find_labeling', 'find_uniques',
                           'global', 'size_filter_blocks', 'write']
    for k in ('size_filter_blocks', 'background_size_filter', 'filling_size_filter'):
        assert cfg[k] == {'threads_per_job': 1, 'time_limit': 60, 'mem_limit': 1., 'qos': 'normal'}


def _chain(task):
    out = []
    while isinstance(task, luigi.Task) and type(task).__name__ != 'DummyTask':
        out.append(task)
        task = task.requires()
    return out


@pytest.mark.parametrize('fill', [False, True])
@pytest.mark.parametrize('relabel', [True, False])
def test_workflow_task_graph(fill, relabel):
    kw = dict(hmap_path='h.n5', hmap_key='hmap') if fill else {}
    wf = SizeFilterWorkflow(tmp_folder='tmp', max_jobs=3, config_dir='cfg', target='local', input_path='a.n5',
                            input_key='seg', output_path='b.n5', output_key='out', size_threshold=25,
                            relabel=relabel, **kw)
    assert wf.hmap_path == ('h.n5' if fill else '') and wf.relabel is relabel
    chain = _chain(wf.requires())
    names = [type(t).__name__ for t in chain]
    filt = 'FillingSizeFilterLocal' if fill else 'BackgroundSizeFilterLocal'
    tail = [filt, 'SizeFilterBlocksLocal', 'FindUniquesLocal']
    assert names == (['RelabelWorkflow', 'WriteLocal', 'FindLabelingLocal', 'FindUniquesLocal'] if relabel else []) + tail
    uniques, blocks, filter_task = chain[-1], chain[-2], chain[-3]
    assert uniques.return_counts is True and (uniques.input_path, uniques.input_key) == ('a.n5', 'seg')
    assert blocks.size_threshold == 25 and (blocks.input_path, blocks.input_key) == ('a.n5', 'seg')
    assert (filter_task.input_path, filter_task.input_key, filter_task.output_path, filter_task.output_key) == \
        ('a.n5', 'seg', 'b.n5', 'out')
    if fill:
        assert (filter_task.hmap_path, filter_task.hmap_key) == ('h.n5', 'hmap')
    if relabel:
        rl = chain[0]
        assert (rl.input_path, rl.input_key, rl.assignment_path, rl.assignment_key) == \
            ('b.n5', 'out', 'b.n5', 'relabel_size_filter')
        assert chain[3].return_counts is False


def test_workflow_defaults_and_hmap_key_check():
    wf = SizeFilterWorkflow(tmp_folder='tmp', max_jobs=1, config_dir='cfg', target='slurm', input_path='a.n5',
                            input_key='seg', output_path='a.n5', output_key='seg', size_threshold=5)
    assert wf.relabel is True and wf.hmap_path == '' and wf.hmap_key == ''
    assert type(_chain(wf.requires())[-3]).__name__ == 'BackgroundSizeFilterSlurm'
    bad = SizeFilterWorkflow(tmp_folder='tmp', max_jobs=1, config_dir='cfg', target='local', input_path='a.n5',
                             input_key='seg', output_path='a.n5', output_key='seg', size_threshold=5,
                             hmap_path='h.n5')
    with pytest.raises(AssertionError):
        bad.requires()


def test_filter_tasks_read_the_discard_path_from_the_log(tmp_path):
    res = tmp_path / 'discard_ids.npy'
    np.save(str(res), np.zeros(0, 'uint64'))
    log = tmp_path / 'size_filter_blocks.log'
    log.write_text('2024-01-01 10:00:00.000001: written config for 1 jobs\n'
                   '2024-01-01 10:00:01.000001: saving results to %s\n'
                   '2024-01-01 10:00:01.000002: size_filter_blocks finished successfully\n'
                   '2024-01-01 10:00:01.000003: Done task size_filter_blocks\n' % str(res))
    assert bg.parse_discard_path(str(log)) == str(res)
    log.write_text('2024-01-01 10:00:01.000003: Done task size_filter_blocks\n')
    with pytest.raises(RuntimeError):
        bg.parse_discard_path(str(log))
