"""CPU tests of the NodeLabelWorkflow task surface (cluster_tools/node_labels/
node_label_workflow.py:8-59, block_node_labels.py, merge_node_labels.py): class names, parameters,
config keys, job and log names with and without prefix, the missing-maxId error, the refusal of
max_overlap with serialize_counts and the serialization.  No GPU call is made."""
import os

import numpy as np
import pytest

from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import _Paths
from cluster_tools_amd.io import File
from cluster_tools_amd.node_labels import NodeLabelWorkflow
from cluster_tools_amd.node_labels import block_node_labels as block
from cluster_tools_amd.node_labels import merge_node_labels as merge
from cluster_tools_amd.node_labels import serialization as S
import node_labels_ref as R

COMMON = {'threads_per_job': 1, 'time_limit': 60, 'mem_limit': 1., 'qos': 'normal'}
TASK = ['tmp_folder', 'max_jobs', 'config_dir']


def _names(cls):
    return [n for n, _ in cls.get_params()]


def _defaults(cls):
    return {n: p.default for n, p in cls.get_params() if n in ('prefix', 'max_overlap', 'ignore_label',
                                                               'serialize_counts')}


def test_task_names_and_parameters():
    assert block.BlockNodeLabelsLocal.task_name == 'block_node_labels'
    assert merge.MergeNodeLabelsLocal.task_name == 'merge_node_labels'
    assert merge.MergeNodeLabelsLocal.allow_retry is False and block.BlockNodeLabelsLocal.allow_retry is True
    for mod, base in ((block, 'BlockNodeLabels'), (merge, 'MergeNodeLabels')):
        for target in ('Base', 'Local', 'Slurm', 'LSF'):
            assert hasattr(mod, base + target)
    assert sorted(_names(block.BlockNodeLabelsLocal)) == sorted(
        TASK + ['ws_path', 'ws_key', 'input_path', 'input_key', 'output_path', 'output_key', 'ignore_label',
                'prefix', 'dependency'])
    assert sorted(_names(merge.MergeNodeLabelsLocal)) == sorted(
        TASK + ['input_path', 'input_key', 'output_path', 'output_key', 'max_overlap', 'ignore_label',
                'serialize_counts', 'prefix', 'dependency'])
    assert sorted(_names(NodeLabelWorkflow)) == sorted(
        TASK + ['target', 'dependency', 'ws_path', 'ws_key', 'input_path', 'input_key', 'output_path',
                'output_key', 'prefix', 'max_overlap', 'ignore_label', 'serialize_counts'])
    if not luigi.HAVE_LUIGI:
        assert _defaults(block.BlockNodeLabelsLocal) == {'prefix': '', 'ignore_label': None}
        want = {'prefix': '', 'max_overlap': True, 'ignore_label': None, 'serialize_counts': False}
        assert _defaults(merge.MergeNodeLabelsLocal) == want and _defaults(NodeLabelWorkflow) == want


def test_config_keys():
    assert block.BlockNodeLabelsLocal.default_task_config() == COMMON
    assert merge.MergeNodeLabelsLocal.default_task_config() == COMMON
    cfg = NodeLabelWorkflow.get_config()
    assert sorted(cfg) == ['block_node_labels', 'global', 'merge_node_labels']
    assert cfg['block_node_labels'] == COMMON and cfg['merge_node_labels'] == COMMON


def _workflow(**kwargs):
    args = dict(tmp_folder='tmp', max_jobs=3, config_dir='cfg', target='local', ws_path='ws.n5', ws_key='seg',
                input_path='gt.n5', input_key='gt', output_path='out.n5', output_key='node_labels')
    args.update(kwargs)
    return NodeLabelWorkflow(**args)


@pytest.mark.parametrize('prefix', ['', 'gt'])
def test_job_and_log_names(prefix):
    m = _workflow(prefix=prefix, target='slurm', ignore_label=0).requires()
    b = m.requires()
    assert type(m).__name__ == 'MergeNodeLabelsSlurm' and type(b).__name__ == 'BlockNodeLabelsSlurm'
    assert isinstance(b, luigi.Task) and m.max_jobs == b.max_jobs == 3
    # the block overlaps go to label_overlaps_<prefix> of the output file, the merge reads them there
    assert (b.ws_path, b.ws_key, b.input_path, b.input_key, b.output_path, b.output_key, b.ignore_label, b.prefix) \
        == ('ws.n5', 'seg', 'gt.n5', 'gt', 'out.n5', 'label_overlaps_%s' % prefix, 0, prefix)
    assert (m.input_path, m.input_key, m.output_path, m.output_key, m.max_overlap, m.ignore_label,
            m.serialize_counts, m.prefix) == ('out.n5', 'label_overlaps_%s' % prefix, 'out.n5', 'node_labels', True, 0,
                                              False, prefix)
    # task logs (the luigi targets)
    assert b.output().path == os.path.join('tmp', 'block_node_labels_%s.log' % prefix)
    assert m.output().path == os.path.join('tmp', 'merge_node_labels_max_ol_%s.log' % prefix)
    all_ol = _workflow(prefix=prefix, max_overlap=False).requires()
    assert all_ol.output().path == os.path.join('tmp', 'merge_node_labels_all_ol_%s.log' % prefix)
    assert all_ol.ignore_label is None and all_ol.requires().ignore_label is None
    # job configs and job logs: the block jobs run under `prefix`, the merge jobs under max_ol_ / all_ol_ + prefix
    p = _Paths('tmp', b.task_name, b.prefix)
    assert p.config(1) == os.path.join('tmp', 'block_node_labels_job_%s_1.config' % prefix)
    assert p.log(1) == os.path.join('tmp', 'logs', 'block_node_labels_%s_1.log' % prefix)
    p = _Paths('tmp', m.task_name, m._job_prefix())
    assert p.config(0) == os.path.join('tmp', 'merge_node_labels_job_max_ol_%s_0.config' % prefix)
    assert p.log(0) == os.path.join('tmp', 'logs', 'merge_node_labels_max_ol_%s_0.log' % prefix)
    assert all_ol._job_prefix() == 'all_ol_%s' % prefix


def _block_task(tmp_path, ws_path):
    cfg = tmp_path / 'cfg'
    cfg.mkdir(exist_ok=True)
    return block.BlockNodeLabelsLocal(tmp_folder=str(tmp_path / 'tmp'), max_jobs=1, config_dir=str(cfg),
                                      ws_path=ws_path, ws_key='seg', input_path=ws_path, input_key='gt',
                                      output_path=str(tmp_path / 'out.n5'), output_key='ol', dependency=None)


def test_missing_max_id(tmp_path):
    ws_path = str(tmp_path / 'ws.n5')
    f = File(ws_path)
    f.create_dataset('seg', data=np.ones((4, 4, 4), 'uint64'), chunks=(4, 4, 4))
    f.create_dataset('gt', data=np.ones((4, 4, 4), 'uint64'), chunks=(4, 4, 4))
    task = _block_task(tmp_path, ws_path)
    task.make_dirs()
    with pytest.raises(KeyError, match='Dataset %s:seg does not have attribute maxId' % ws_path):
        task.run_impl()
    assert not os.path.exists(str(tmp_path / 'out.n5'))  # nothing was created, no job ran
    assert not [n for n in os.listdir(str(tmp_path / 'tmp')) if n.endswith('.config')]


def test_max_overlap_with_counts_is_refused(tmp_path):
    merge.check_supported(True, False)
    merge.check_supported(False, True)
    merge.check_supported(False, False)
    with pytest.raises(NotImplementedError, match='serialize_counts'):
        merge.check_supported(True, True)
    with pytest.raises(NotImplementedError, match='serialize_counts'):
        _workflow(max_overlap=True, serialize_counts=True).requires()
    # the task refuses in run_impl before it reads its input or writes a job config
    cfg = tmp_path / 'cfg'
    cfg.mkdir()
    task = merge.MergeNodeLabelsLocal(tmp_folder=str(tmp_path / 'tmp'), max_jobs=1, config_dir=str(cfg),
                                      input_path=str(tmp_path / 'no.n5'), input_key='ol',
                                      output_path=str(tmp_path / 'out.n5'), output_key='nl', max_overlap=True,
                                      serialize_counts=True, dependency=None)
    task.make_dirs()
    with pytest.raises(NotImplementedError, match='serialize_counts'):
        task.run_impl()
    assert not os.path.exists(str(tmp_path / 'out.n5'))
    assert not [n for n in os.listdir(str(tmp_path / 'tmp')) if n.endswith('.config')]


def _rows(seed):
    rng = np.random.RandomState(seed)
    nodes = rng.randint(0, 9, (4, 5, 6)).astype(np.uint64) * np.uint64(2 ** 33 + 1)
    labels = rng.randint(0, 5, (4, 5, 6)).astype(np.uint64)
    labels[0, 0, :3] = 2 ** 64 - 1
    return R.overlap_rows(nodes, labels)


def test_serialization_layout():
    rows = np.array([[2, 1, 10], [2, 5, 3], [7, 4, 1]], 'uint64')
    assert S.serialize_overlaps(rows).tolist() == [2, 2, 1, 10, 5, 3, 7, 1, 4, 1]
    assert S.serialize_overlaps(rows, with_counts=False).tolist() == [2, 2, 1, 5, 7, 1, 4]
    assert S.serialize_overlaps(np.zeros((0, 3), 'uint64')).shape == (0,)
    assert S.deserialize_overlaps(np.zeros(0, 'uint64')).shape == (0, 3)
    for bad in ([2], [2, 2, 1, 10, 5], [2, 1, 1, 10, 9]):
        with pytest.raises(ValueError, match='overlap chunk'):
            S.deserialize_overlaps(np.array(bad, 'uint64'))


@pytest.mark.parametrize('with_counts', [True, False])
def test_serialization_round_trip(tmp_path, with_counts):
    rows = _rows(0)
    flat = S.serialize_overlaps(rows, with_counts)
    assert flat.dtype == np.uint64 and flat.ndim == 1
    want = rows.copy()
    if not with_counts:
        want[:, 2] = 0
    np.testing.assert_array_equal(S.deserialize_overlaps(flat, with_counts), want)
    # through a dataset, as the tasks write it
    ds = File(str(tmp_path / 'a.n5')).create_dataset('ol', shape=(8, 8, 8), chunks=(4, 4, 4), dtype='uint64')
    if not with_counts:
        ds.attrs[S.COUNTS_ATTR] = False
    ds.write_chunk((1, 0, 1), flat, True)
    d, max_label = S.deserialize_overlap_chunk(ds.path, (1, 0, 1))
    assert d == R.rows_to_dict(want) and max_label == 2 ** 64 - 1
    assert all(isinstance(k, int) for k in d)
    np.testing.assert_array_equal(S.read_overlap_rows(ds, (1, 0, 1), with_counts), want)


def test_deserialize_a_missing_chunk(tmp_path):
    ds = File(str(tmp_path / 'a.n5')).create_dataset('ol', shape=(8, 8, 8), chunks=(4, 4, 4), dtype='uint64')
    assert S.deserialize_overlap_chunk(ds.path, (0, 1, 1)) == ({}, 0)
    assert S.read_overlap_rows(ds, (0, 1, 1)).shape == (0, 3)
    ds.write_chunk((0, 0, 0), np.zeros((4, 4, 4), 'uint64'))  # a fixed-size chunk is no overlap chunk
    with pytest.raises(ValueError, match='variable-length'):
        S.deserialize_overlap_chunk(ds.path, (0, 0, 0))


def test_max_overlap_labels_of_a_node_range():
    rows = _rows(1)
    rows[:, 0] //= np.uint64(2 ** 33 + 1)  # nodes 0..8
    full = R.max_overlap(rows, 12, 3)
    np.testing.assert_array_equal(merge.max_overlap_labels(rows, 0, 12, 3), full)
    sel = rows[(rows[:, 0] >= 4) & (rows[:, 0] < 10)]
    np.testing.assert_array_equal(merge.max_overlap_labels(sel, 4, 10, None), R.max_overlap(rows, 12, None)[4:10])
    assert merge.max_overlap_labels(np.zeros((0, 3), 'uint64'), 5, 8, 9).tolist() == [9, 9, 9]
    # a tie: the smallest label wins
    tie = np.array([[6, 8, 4], [6, 2, 4], [6, 1, 3]], 'uint64')
    assert merge.max_overlap_labels(tie, 6, 7, None).tolist() == [2]
