"""CPU tests of the lifted-feature task surface (cluster_tools/lifted_features/*.py): class names,
parameters, task names, config keys, the task graph of LiftedFeaturesFromNodeLabelsWorkflow with and
without clear labels, the refusal of label_overlap_threshold, and the host jobs (costs, clear,
merge) in-process on small n5 inputs against the restated rules (tests/lifted_features_ref.py).
No GPU call is made."""
import json
import os

import numpy as np
import pytest

from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import _Paths
from cluster_tools_amd.io import File
from cluster_tools_amd.lifted_features import LiftedFeaturesFromNodeLabelsWorkflow
from cluster_tools_amd.lifted_features import sparse_lifted_neighborhood as nh
from cluster_tools_amd.lifted_features import costs_from_node_labels as costs
from cluster_tools_amd.lifted_features import clear_lifted_edges_from_labels as clear
from cluster_tools_amd.lifted_features import merge_lifted_problems as merge
import lifted_features_ref as R

COMMON = {'threads_per_job': 1, 'time_limit': 60, 'mem_limit': 1., 'qos': 'normal'}
TASK = ['tmp_folder', 'max_jobs', 'config_dir']


def _names(cls):
    return sorted(n for n, _ in cls.get_params())


def test_class_names_task_names_and_retry():
    for mod, base, name in ((nh, 'SparseLiftedNeighborhood', 'sparse_lifted_neighborhood'),
                            (costs, 'CostsFromNodeLabels', 'costs_from_node_labels'),
                            (clear, 'ClearLiftedEdgesFromLabels', 'clear_lifted_edges_from_labels'),
                            (merge, 'MergeLiftedProblems', 'merge_lifted_problems')):
        for target in ('Base', 'Local', 'Slurm', 'LSF'):
            cls = getattr(mod, base + target)
            assert cls.task_name == name and cls.allow_retry is False
            assert os.path.samefile(cls.src_file, mod.__file__)
    assert nh.SparseLiftedNeighborhoodBase.modes == ('all', 'same', 'different')
    import cluster_tools_amd.lifted_features as pkg
    assert pkg.LiftedFeaturesFromNodeLabelsWorkflow is LiftedFeaturesFromNodeLabelsWorkflow


def test_parameters():
    assert _names(nh.SparseLiftedNeighborhoodLocal) == sorted(
        TASK + ['graph_path', 'graph_key', 'node_label_path', 'node_label_key', 'output_path', 'output_key',
                'prefix', 'nh_graph_depth', 'node_ignore_label', 'mode', 'dependency'])
    assert _names(costs.CostsFromNodeLabelsLocal) == sorted(
        TASK + ['nh_path', 'nh_key', 'node_label_path', 'node_label_key', 'output_path', 'output_key', 'prefix',
                'dependency'])
    assert _names(clear.ClearLiftedEdgesFromLabelsLocal) == sorted(
        TASK + ['node_labels_path', 'node_labels_key', 'lifted_edge_path', 'lifted_edge_key', 'dependency'])
    assert _names(merge.MergeLiftedProblemsLocal) == sorted(TASK + ['path', 'prefixs', 'out_prefix', 'dependency'])
    assert _names(LiftedFeaturesFromNodeLabelsWorkflow) == sorted(
        TASK + ['target', 'dependency', 'ws_path', 'ws_key', 'labels_path', 'labels_key', 'graph_path', 'graph_key',
                'output_path', 'nh_out_key', 'feat_out_key', 'prefix', 'nh_graph_depth', 'ignore_label',
                'label_ignore_label', 'label_overlap_threshold', 'clear_labels_path', 'clear_labels_key', 'mode'])
    if not luigi.HAVE_LUIGI:
        d = {n: p.default for n, p in LiftedFeaturesFromNodeLabelsWorkflow.get_params()}
        assert (d['nh_graph_depth'], d['ignore_label'], d['label_ignore_label'], d['label_overlap_threshold'],
                d['clear_labels_path'], d['clear_labels_key'], d['mode']) == (4, 0, None, None, None, None, 'all')
        d = {n: p.default for n, p in nh.SparseLiftedNeighborhoodLocal.get_params()}
        assert d['node_ignore_label'] == 0 and d['mode'] == 'all'


def test_config_keys():
    assert nh.SparseLiftedNeighborhoodLocal.default_task_config() == COMMON
    assert clear.ClearLiftedEdgesFromLabelsLocal.default_task_config() == COMMON
    assert merge.MergeLiftedProblemsLocal.default_task_config() == COMMON
    assert costs.CostsFromNodeLabelsLocal.default_task_config() == dict(COMMON, intra_label_cost=6.,
                                                                         inter_label_cost=-6.)
    cfg = LiftedFeaturesFromNodeLabelsWorkflow.get_config()
    assert sorted(cfg) == ['block_node_labels', 'clear_lifted_edges_from_labels', 'features_from_node_labels',
                           'global', 'merge_node_labels', 'sparse_lifted_neighborhood']
    assert cfg['features_from_node_labels'] == costs.CostsFromNodeLabelsLocal.default_task_config()
    assert cfg['sparse_lifted_neighborhood'] == COMMON and cfg['clear_lifted_edges_from_labels'] == COMMON


def _workflow(**kwargs):
    args = dict(tmp_folder='tmp', max_jobs=3, config_dir='cfg', target='slurm', ws_path='ws.n5', ws_key='seg',
                labels_path='gt.n5', labels_key='gt', graph_path='graph.n5', graph_key='s0/graph',
                output_path='out.n5', nh_out_key='lifted_nh', feat_out_key='lifted_costs', prefix='nuc')
    args.update(kwargs)
    return LiftedFeaturesFromNodeLabelsWorkflow(**args)


def _chain(task):
    """The tasks from the last one back to the first, workflows opened."""
    names = []
    while isinstance(task, luigi.Task) and type(task).__name__ != 'DummyTask':
        names.append(task)
        task = task.requires()
    return names


def test_task_graph_without_clear_labels():
    chain = _chain(_workflow(nh_graph_depth=3, mode='different', ignore_label=5, label_ignore_label=0).requires())
    assert [type(t).__name__ for t in chain] == [
        'CostsFromNodeLabelsSlurm', 'SparseLiftedNeighborhoodSlurm', 'NodeLabelWorkflow', 'MergeNodeLabelsSlurm',
        'BlockNodeLabelsSlurm']
    cost, lifted, labels = chain[0], chain[1], chain[2]
    assert all(t.max_jobs == 3 and t.tmp_folder == 'tmp' and t.config_dir == 'cfg' for t in chain)
    assert (cost.nh_path, cost.nh_key, cost.node_label_path, cost.node_label_key, cost.output_path, cost.output_key,
            cost.prefix) == ('out.n5', 'lifted_nh', 'out.n5', 'node_overlaps/nuc', 'out.n5', 'lifted_costs', 'nuc')
    assert (lifted.graph_path, lifted.graph_key, lifted.node_label_path, lifted.node_label_key, lifted.output_path,
            lifted.output_key, lifted.nh_graph_depth, lifted.mode, lifted.prefix, lifted.node_ignore_label) == (
        'graph.n5', 's0/graph', 'out.n5', 'node_overlaps/nuc', 'out.n5', 'lifted_nh', 3, 'different', 'nuc', 5)
    assert (labels.target, labels.ws_path, labels.ws_key, labels.input_path, labels.input_key, labels.output_path,
            labels.output_key, labels.prefix, labels.max_overlap, labels.serialize_counts, labels.ignore_label) == (
        'slurm', 'ws.n5', 'seg', 'gt.n5', 'gt', 'out.n5', 'node_overlaps/nuc', 'nuc', True, False, 0)
    # logs and job files run under the prefix
    assert cost.output().path == os.path.join('tmp', 'costs_from_node_labels_nuc.log')
    assert lifted.output().path == os.path.join('tmp', 'sparse_lifted_neighborhood_nuc.log')
    p = _Paths('tmp', lifted.task_name, lifted.prefix)
    assert p.config(0) == os.path.join('tmp', 'sparse_lifted_neighborhood_job_nuc_0.config')
    assert p.log(0) == os.path.join('tmp', 'logs', 'sparse_lifted_neighborhood_nuc_0.log')


def test_task_graph_with_clear_labels():
    chain = _chain(_workflow(clear_labels_path='clear.n5', clear_labels_key='cells', target='local').requires())
    assert [type(t).__name__ for t in chain] == [
        'CostsFromNodeLabelsLocal', 'ClearLiftedEdgesFromLabelsLocal', 'NodeLabelWorkflow', 'MergeNodeLabelsLocal',
        'BlockNodeLabelsLocal', 'SparseLiftedNeighborhoodLocal', 'NodeLabelWorkflow', 'MergeNodeLabelsLocal',
        'BlockNodeLabelsLocal']
    clr, clear_labels, lifted = chain[1], chain[2], chain[5]
    assert (clr.node_labels_path, clr.node_labels_key, clr.lifted_edge_path, clr.lifted_edge_key) == (
        'out.n5', 'node_overlaps/clear_nuc', 'out.n5', 'lifted_nh')
    assert clr.output().path == os.path.join('tmp', 'clear_lifted_edges_from_labels.log')
    assert (clear_labels.input_path, clear_labels.input_key, clear_labels.output_key, clear_labels.prefix,
            clear_labels.max_overlap, clear_labels.ignore_label) == (
        'clear.n5', 'cells', 'node_overlaps/clear_nuc', 'clear_nuc', True, None)
    assert lifted.nh_graph_depth == 4 and lifted.mode == 'all' and lifted.node_ignore_label == 0
    with pytest.raises(AssertionError):
        _workflow(clear_labels_path='clear.n5').requires()


def test_label_overlap_threshold_is_refused():
    with pytest.raises(NotImplementedError, match='label_overlap_threshold'):
        _workflow(label_overlap_threshold=0.5).requires()
    assert not hasattr(__import__('cluster_tools_amd.lifted_features.lifted_feature_workflow', fromlist=['x']),
                       'NodeLabelsWithThreshold')


# ---- the host jobs, in-process ---------------------------------------------------------------

NODE_LABELS = np.array([0, 3, 3, 2 ** 40, 2 ** 40 + 2 ** 32, 3, 7, 7], dtype='uint64')
LIFTED = np.array([[1, 2], [1, 3], [1, 5], [2, 6], [3, 4], [6, 7]], dtype='uint64')


def _job_config(tmp_path, name, **config):
    path = str(tmp_path / ('%s_job_0.config' % name))
    with open(path, 'w') as f:
        json.dump(config, f)
    return path


def _problem(tmp_path, lifted=LIFTED, chunks=(4, 2)):
    path = str(tmp_path / 'out.n5')
    f = File(path)
    f.create_dataset('labels', data=NODE_LABELS, chunks=(8,))
    f.create_dataset('lifted_nh', data=lifted, chunks=chunks)
    return path


def test_costs_job(tmp_path):
    path = _problem(tmp_path)
    File(path).create_dataset('costs', shape=(6,), chunks=(4,), dtype='float32')
    cfg = dict(nh_path=path, nh_key='lifted_nh', node_label_path=path, node_label_key='labels', output_path=path,
               output_key='costs', chunk_size=4, intra_label_cost=6., inter_label_cost=-6.)
    costs.costs_from_node_labels(0, _job_config(tmp_path, 'a', block_list=[0, 1], **cfg))
    ds = File(path)['costs']
    got = ds[:]
    assert str(ds.dtype) == 'float32' and got.tolist() == [6., -6., 6., -6., -6., 6.]
    np.testing.assert_array_equal(got, R.lifted_costs(LIFTED, NODE_LABELS))
    # other costs, and only the job's edge blocks are written
    cfg.update(output_key='costs2', intra_label_cost=1.25, inter_label_cost=-0.5)
    File(path).create_dataset('costs2', shape=(6,), chunks=(4,), dtype='float32')
    costs.costs_from_node_labels(1, _job_config(tmp_path, 'b', block_list=[1], **cfg))
    want = R.lifted_costs(LIFTED, NODE_LABELS, 1.25, -0.5)
    want[:4] = 0
    np.testing.assert_array_equal(File(path)['costs2'][:], want)


def test_costs_job_refuses_an_unlabelled_endpoint(tmp_path):
    lifted = np.array([[1, 2], [0, 5]], dtype='uint64')
    path = _problem(tmp_path, lifted, chunks=(2, 2))
    File(path).create_dataset('costs', shape=(2,), chunks=(2,), dtype='float32')
    cfg = dict(nh_path=path, nh_key='lifted_nh', node_label_path=path, node_label_key='labels', output_path=path,
               output_key='costs', chunk_size=2, intra_label_cost=6., inter_label_cost=-6., block_list=[0])
    with pytest.raises(ValueError, match='label 0'):
        costs.costs_from_node_labels(0, _job_config(tmp_path, 'a', **cfg))
    with pytest.raises(ValueError):
        R.lifted_costs(lifted, NODE_LABELS)


def _mtimes(root):
    return {os.path.join(d, n): os.stat(os.path.join(d, n)).st_mtime_ns for d, _, names in os.walk(root)
            for n in names}


def test_clear_job(tmp_path):
    path = _problem(tmp_path)
    clear_labels = np.array([1, 1, 1, 1, 2, 2, 1, 2], dtype='uint64')
    File(path).create_dataset('clear', data=clear_labels, chunks=(8,))
    cfg = _job_config(tmp_path, 'c', node_labels_path=path, node_labels_key='clear', lifted_edge_path=path,
                      lifted_edge_key='lifted_nh')
    clear.clear_lifted_edges_from_labels(0, cfg)
    ds = File(path)['lifted_nh']
    want = R.clear_lifted_edges(LIFTED, clear_labels)
    assert want.tolist() == [[1, 2], [1, 3], [2, 6]]
    np.testing.assert_array_equal(ds[:], want)
    assert str(ds.dtype) == 'uint64' and tuple(ds.chunks) == (3, 2)  # the old chunks, cut to the new extent
    # nothing is dropped: the dataset is not written again
    before = _mtimes(os.path.join(path, 'lifted_nh'))
    clear.clear_lifted_edges_from_labels(0, cfg)
    assert _mtimes(os.path.join(path, 'lifted_nh')) == before
    np.testing.assert_array_equal(File(path)['lifted_nh'][:], want)


def test_clear_job_refuses_to_drop_every_edge(tmp_path):
    path = _problem(tmp_path)
    File(path).create_dataset('clear', data=np.arange(8, dtype='uint64'), chunks=(8,))
    before = _mtimes(os.path.join(path, 'lifted_nh'))
    with pytest.raises(RuntimeError, match='nothing to write'):
        clear.clear_lifted_edges_from_labels(0, _job_config(
            tmp_path, 'c', node_labels_path=path, node_labels_key='clear', lifted_edge_path=path,
            lifted_edge_key='lifted_nh'))
    assert _mtimes(os.path.join(path, 'lifted_nh')) == before


def test_merge_job_keeps_duplicates(tmp_path):
    path = str(tmp_path / 'problem.n5')
    f = File(path)
    a = np.array([[1, 4], [2, 9]], dtype='uint64')
    b = np.array([[0, 3], [1, 4], [5, 6]], dtype='uint64')
    for prefix, e, c in (('nuc', a, [6., -6.]), ('sem', b, [-6., -6., 6.])):
        f.create_dataset('s0/lifted_nh_%s' % prefix, data=e, chunks=(len(e), 2))
        f.create_dataset('s0/lifted_costs_%s' % prefix, data=np.array(c, dtype='float32'), chunks=(len(e),))
    merge.merge_lifted_problems(0, _job_config(tmp_path, 'm', path=path, prefixs=['nuc', 'sem'], out_prefix='all'))
    e, c = File(path)['s0/lifted_nh_all'], File(path)['s0/lifted_costs_all']
    # concatenated in the order of the prefixes; the shared edge (1, 4) stays twice with both costs
    np.testing.assert_array_equal(e[:], np.concatenate([a, b]))
    assert c[:].tolist() == [6., -6., -6., -6., 6.]
    assert str(e.dtype) == 'uint64' and str(c.dtype) == 'float32'
    assert tuple(e.chunks) == (5, 2) and tuple(c.chunks) == (5,)
    t = merge.MergeLiftedProblemsLocal(tmp_folder='tmp', max_jobs=1, config_dir='cfg', path=path,
                                       prefixs=['nuc', 'sem'], out_prefix='all', dependency=None)
    assert t.output().path == os.path.join('tmp', 'merge_lifted_problems_all.log')


def test_lifted_edges_dataset_layout(tmp_path):
    f = File(str(tmp_path / 'o.n5'))
    ds = nh.write_lifted_edges(f, 'nh', LIFTED)
    assert tuple(ds.shape) == (6, 2) and tuple(ds.chunks) == (6, 2) and str(ds.dtype) == 'uint64'
    big = np.stack([np.zeros(300000, dtype='uint64'), np.arange(300000, dtype='uint64')], axis=1)
    ds = nh.write_lifted_edges(f, 'nh', big)  # a table of an earlier run is replaced
    assert tuple(ds.shape) == (300000, 2) and tuple(ds.chunks) == (262144, 2)
    np.testing.assert_array_equal(f['nh'][299990:], big[299990:])
    with pytest.raises(AssertionError):
        nh.write_lifted_edges(f, 'empty', np.zeros((0, 2), dtype='uint64'))
