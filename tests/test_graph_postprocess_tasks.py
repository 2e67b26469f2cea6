"""CPU tests of the graph postprocessing's task surface (cluster_tools/postprocess/
graph_connected_components.py, graph_watershed_assignments.py, postprocess_workflow.py:296-427):
class names, parameters and defaults, default configs, the job configs the tasks write, the task
graphs of ConnectedComponentsWorkflow and SizeFilterAndGraphWatershedWorkflow with and without the
Write step, and the job's host side up to the GPU call: what it reads, the seeds it builds and the
assertions that fire before a handle is opened.  No GPU call is made."""
import json
import os

import numpy as np
import pytest

from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import _Paths
from cluster_tools_amd.io import File
from cluster_tools_amd.graph.serialization import write_graph
from cluster_tools_amd.postprocess import (ConnectedComponentsWorkflow, SizeFilterAndGraphWatershedWorkflow,
                                           SizeFilterWorkflow)
from cluster_tools_amd.postprocess import graph_connected_components as cc
from cluster_tools_amd.postprocess import graph_watershed_assignments as gws
from cluster_tools_amd.postprocess import postprocess_workflow
import graph_postprocess_ref as R

COMMON = {'threads_per_job': 1, 'time_limit': 60, 'mem_limit': 1., 'qos': 'normal'}
TASK = ['tmp_folder', 'max_jobs', 'config_dir']


def _names(cls):
    return sorted(n for n, _ in cls.get_params())


def test_class_names_task_names_and_retry():
    for mod, base, name in ((cc, 'GraphConnectedComponents', 'graph_connected_components'),
                            (gws, 'GraphWatershedAssignments', 'graph_watershed_assignments')):
        for target in ('Base', 'Local', 'Slurm', 'LSF'):
            cls = getattr(mod, base + target)
            assert cls.task_name == name and cls.allow_retry is False
            assert os.path.samefile(cls.src_file, mod.__file__)
    assert postprocess_workflow.ConnectedComponentsWorkflow is ConnectedComponentsWorkflow
    assert postprocess_workflow.SizeFilterAndGraphWatershedWorkflow is SizeFilterAndGraphWatershedWorkflow
    assert postprocess_workflow.SizeFilterWorkflow is SizeFilterWorkflow
    for name in ('FilterOrphansWorkflow', 'FilterLabelsWorkflow', 'FilterByThresholdWorkflow'):
        assert not hasattr(postprocess_workflow, name)


def test_parameters_and_defaults():
    assert _names(cc.GraphConnectedComponentsLocal) == sorted(
        TASK + ['problem_path', 'graph_key', 'assignment_path', 'assignment_key', 'output_path', 'output_key',
                'dependency'])
    assert _names(gws.GraphWatershedAssignmentsLocal) == sorted(
        TASK + ['problem_path', 'graph_key', 'features_key', 'filter_nodes_path', 'assignment_path', 'assignment_key',
                'output_path', 'output_key', 'relabel', 'from_costs', 'dependency'])
    assert _names(ConnectedComponentsWorkflow) == sorted(
        TASK + ['target', 'dependency', 'problem_path', 'graph_key', 'path', 'fragments_key', 'assignment_path',
                'assignment_key', 'output_path', 'assignment_out_key', 'output_key'])
    assert _names(SizeFilterAndGraphWatershedWorkflow) == sorted(
        TASK + ['target', 'dependency', 'problem_path', 'graph_key', 'features_key', 'path', 'segmentation_key',
                'fragments_key', 'assignment_key', 'size_threshold', 'relabel', 'from_costs', 'output_path',
                'assignment_out_key', 'output_key'])
    if not luigi.HAVE_LUIGI:
        d = {n: p.default for n, p in gws.GraphWatershedAssignmentsLocal.get_params()}
        assert (d['relabel'], d['from_costs']) == (False, True)
        d = {n: p.default for n, p in SizeFilterAndGraphWatershedWorkflow.get_params()}
        assert (d['relabel'], d['from_costs'], d['fragments_key'], d['output_key']) == (False, False, '', '')
        d = {n: p.default for n, p in ConnectedComponentsWorkflow.get_params()}
        assert (d['fragments_key'], d['output_key']) == ('', '')


def test_config_keys():
    assert cc.GraphConnectedComponentsLocal.default_task_config() == COMMON
    assert gws.GraphWatershedAssignmentsLocal.default_task_config() == COMMON
    cfg = ConnectedComponentsWorkflow.get_config()
    assert sorted(cfg) == ['global', 'graph_connected_components', 'write']
    assert cfg['graph_connected_components'] == COMMON
    assert cfg['write'] == dict(COMMON, chunks=None, allow_empty_assignments=False)
    cfg = SizeFilterAndGraphWatershedWorkflow.get_config()
    assert sorted(cfg) == ['find_uniques', 'global', 'graph_watershed_assignments', 'size_filter_blocks', 'write']
    assert cfg['graph_watershed_assignments'] == COMMON and cfg['size_filter_blocks'] == COMMON


def _stubbed(cls):
    """The task class with the job run taken out: run_impl only writes the script and the job config."""
    class Stub(cls):
        def submit_jobs(self, n_jobs, job_prefix=None):
            assert n_jobs == 1 and job_prefix is None

        def wait_for_jobs(self, job_prefix=None):
            pass

        def check_jobs(self, n_jobs, job_prefix=None):
            assert n_jobs == 1 and job_prefix is None
    Stub.__name__ = cls.__name__
    return Stub


def _job_config_of(task):
    task.make_dirs()
    task.run_impl()
    paths = _Paths(task.tmp_folder, task.task_name)
    assert os.path.exists(paths.script())
    assert not os.path.exists(paths.config(1))
    with open(paths.config(0)) as f:
        return json.load(f)


def test_job_configs(tmp_path):
    common = dict(tmp_folder=str(tmp_path / 'tmp'), max_jobs=4, config_dir=str(tmp_path / 'cfg'), dependency=None)
    task = _stubbed(cc.GraphConnectedComponentsLocal)(
        problem_path='p.n5', graph_key='s0/graph', assignment_path='a.n5', assignment_key='ass', output_path='o.n5',
        output_key='cc', **common)
    assert _job_config_of(task) == dict(COMMON, problem_path='p.n5', graph_key='s0/graph', assignment_path='a.n5',
                                        assignment_key='ass', output_path='o.n5', output_key='cc')
    assert task.output().path == os.path.join(common['tmp_folder'], 'graph_connected_components.log')
    task = _stubbed(gws.GraphWatershedAssignmentsLocal)(
        problem_path='p.n5', graph_key='s0/graph', features_key='feats', filter_nodes_path='tmp/discard_ids.npy',
        assignment_path='a.n5', assignment_key='ass', output_path='o.n5', output_key='gws', relabel=True, **common)
    assert _job_config_of(task) == dict(
        COMMON, problem_path='p.n5', graph_key='s0/graph', features_key='feats',
        filter_nodes_path='tmp/discard_ids.npy', assignment_path='a.n5', assignment_key='ass', output_path='o.n5',
        output_key='gws', relabel=True, from_costs=True)
    # a task config in config_dir is read
    os.makedirs(common['config_dir'])
    with open(os.path.join(common['config_dir'], 'graph_watershed_assignments.config'), 'w') as f:
        json.dump(dict(COMMON, threads_per_job=4), f)
    task = _stubbed(gws.GraphWatershedAssignmentsLocal)(
        problem_path='p.n5', graph_key='g', features_key='f', filter_nodes_path='d.npy', assignment_path='a.n5',
        assignment_key='ass', output_path='o.n5', output_key='gws', from_costs=False, **common)
    cfg = _job_config_of(task)
    assert cfg['threads_per_job'] == 4 and cfg['from_costs'] is False and cfg['relabel'] is False


def _chain(task):
    """The tasks from the last one back to the first, workflows opened."""
    tasks = []
    while isinstance(task, luigi.Task) and type(task).__name__ != 'DummyTask':
        tasks.append(task)
        task = task.requires()
    return tasks


def _cc_workflow(**kwargs):
    args = dict(tmp_folder='tmp', max_jobs=3, config_dir='cfg', target='slurm', problem_path='p.n5',
                graph_key='s0/graph', path='data.n5', assignment_path='a.n5', assignment_key='ass',
                output_path='out.n5', assignment_out_key='cc_ass')
    args.update(kwargs)
    return ConnectedComponentsWorkflow(**args)


def test_connected_components_workflow_graph():
    chain = _chain(_cc_workflow().requires())
    assert [type(t).__name__ for t in chain] == ['GraphConnectedComponentsSlurm']
    t = chain[0]
    assert (t.tmp_folder, t.max_jobs, t.config_dir) == ('tmp', 3, 'cfg')
    assert (t.problem_path, t.graph_key, t.assignment_path, t.assignment_key, t.output_path, t.output_key) == (
        'p.n5', 's0/graph', 'a.n5', 'ass', 'out.n5', 'cc_ass')
    chain = _chain(_cc_workflow(output_key='seg_cc', fragments_key='frags', target='local').requires())
    assert [type(t).__name__ for t in chain] == ['WriteLocal', 'GraphConnectedComponentsLocal']
    w = chain[0]
    assert (w.input_path, w.input_key, w.output_path, w.output_key, w.assignment_path, w.assignment_key,
            w.identifier) == ('data.n5', 'frags', 'out.n5', 'seg_cc', 'out.n5', 'cc_ass', 'graph-connected-components')
    assert w.output().path == os.path.join('tmp', 'write_graph-connected-components.log')
    with pytest.raises(AssertionError):
        _cc_workflow(output_key='seg_cc').requires()


def _gws_workflow(**kwargs):
    args = dict(tmp_folder='tmp', max_jobs=3, config_dir='cfg', target='lsf', problem_path='p.n5', graph_key='s0/graph',
                features_key='feats', path='data.n5', segmentation_key='seg', assignment_key='ass', size_threshold=100,
                output_path='out.n5', assignment_out_key='gws_ass')
    args.update(kwargs)
    return SizeFilterAndGraphWatershedWorkflow(**args)


def test_graph_watershed_workflow_graph():
    chain = _chain(_gws_workflow().requires())
    assert [type(t).__name__ for t in chain] == ['GraphWatershedAssignmentsLSF', 'SizeFilterBlocksLSF', 'FindUniquesLSF']
    g, sf, un = chain
    assert all((t.tmp_folder, t.max_jobs, t.config_dir) == ('tmp', 3, 'cfg') for t in chain)
    assert (g.problem_path, g.graph_key, g.features_key, g.assignment_path, g.assignment_key, g.output_path,
            g.output_key, g.filter_nodes_path, g.relabel, g.from_costs) == (
        'p.n5', 's0/graph', 'feats', 'data.n5', 'ass', 'out.n5', 'gws_ass', os.path.join('tmp', 'discard_ids.npy'),
        False, False)
    assert (sf.input_path, sf.input_key, sf.size_threshold) == ('data.n5', 'seg', 100)
    assert (un.input_path, un.input_key, un.return_counts) == ('data.n5', 'seg', True)
    chain = _chain(_gws_workflow(output_key='seg_out', fragments_key='frags', relabel=True, from_costs=True,
                                 target='local').requires())
    assert [type(t).__name__ for t in chain] == ['WriteLocal', 'GraphWatershedAssignmentsLocal',
                                                 'SizeFilterBlocksLocal', 'FindUniquesLocal']
    w, g = chain[0], chain[1]
    assert (g.relabel, g.from_costs) == (True, True)
    assert (w.input_path, w.input_key, w.output_path, w.output_key, w.assignment_path, w.assignment_key,
            w.identifier) == ('data.n5', 'frags', 'out.n5', 'seg_out', 'out.n5', 'gws_ass', 'size-filter-graph-ws')
    with pytest.raises(AssertionError):
        _gws_workflow(output_key='seg_out').requires()


# ---- the job's host side, in-process ----------------------------------------------------------

EDGES = np.array([[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [5, 6]], dtype='uint64')
COSTS = np.array([.5, .1, .9, .2, .3, .4])
ASSIGNMENTS = np.array([3, 0, 5, 5, 2, 0, 3], dtype='uint64')


def _problem(tmp_path, assignments=ASSIGNMENTS, discard=(5,), features=None, **config):
    path = str(tmp_path / 'problem.n5')
    f = File(path)
    write_graph(f, 's0/graph', np.arange(7, dtype='uint64'), EDGES, True)
    if features is None:  # the merged edge features: the costs are column 0
        features = np.stack([COSTS] + [np.full(len(COSTS), 7.)] * 9, axis=1)
    f.create_dataset('feats', data=features, chunks=features.shape)
    f.create_dataset('ass', data=np.asarray(assignments, dtype='uint64'), chunks=(4,))
    discard_path = str(tmp_path / 'discard_ids.npy')
    np.save(discard_path, np.array(discard, dtype='uint64'))
    cfg = dict(COMMON, problem_path=path, graph_key='s0/graph', features_key='feats', filter_nodes_path=discard_path,
               assignment_path=path, assignment_key='ass', output_path=path, output_key='out', relabel=False,
               from_costs=False)
    cfg.update(config)
    return cfg


def test_load_problem(tmp_path, capsys):
    cfg = _problem(tmp_path)
    edges, weights, seeds, seed_offset, chunks = gws.load_problem(cfg)
    np.testing.assert_array_equal(edges, EDGES)
    np.testing.assert_array_equal(weights, COSTS)
    want_seeds, want_offset = R.task_seeds(ASSIGNMENTS, [5])
    assert seed_offset == want_offset == 6 and seeds.tolist() == want_seeds.tolist() == [3, 6, 0, 0, 2, 6, 3]
    assert tuple(chunks) == (4,) and seeds.dtype == np.uint64
    out = capsys.readouterr().out
    assert 'Read features and edges from %s' % cfg['problem_path'] in out and 'Discarding 2 fragments' in out
    assert 'Mapping costs' not in out
    # from_costs, and a 1-D feature array
    cfg = _problem(tmp_path / 'b', features=COSTS.astype('float32'), from_costs=True)
    weights = gws.load_problem(cfg)[1]
    assert weights.dtype == np.float32
    np.testing.assert_array_equal(weights, R.costs_to_weights(COSTS.astype('float32')))
    assert 'Mapping costs with range 0.100000 to 0.900000 to range 0 to 1' in capsys.readouterr().out


@pytest.fixture
def no_handle(monkeypatch):
    """Any attempt to open a GPU handle fails the test."""
    from cluster_tools_amd import ctws

    def refuse(*args, **kwargs):
        raise RuntimeError("a GPU handle was opened")
    monkeypatch.setattr(ctws, 'Handle', refuse)


def _job_config(tmp_path, cfg):
    path = str(tmp_path / 'graph_watershed_assignments_job_0.config')
    with open(path, 'w') as f:
        json.dump(cfg, f)
    return path


def test_the_assertions_fire_before_any_gpu_call(tmp_path, no_handle):
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    cfg = _problem(tmp_path / 'a', assignments=ASSIGNMENTS[:6])
    with pytest.raises(AssertionError, match='Expected number of nodes 7 and number of assignments 6 does not agree'):
        gws.graph_watershed_assignments(0, _job_config(tmp_path / 'a', cfg))
    cfg = _problem(tmp_path / 'b', discard=(0, 5))
    with pytest.raises(AssertionError, match='Breaks logic'):
        gws.graph_watershed_assignments(0, _job_config(tmp_path / 'b', cfg))
    assert 'out' not in File(cfg['output_path'])
    # (with sound inputs the job gets as far as the handle)
    (tmp_path / 'c').mkdir()
    cfg = _problem(tmp_path / 'c')
    with pytest.raises(RuntimeError, match='a GPU handle was opened'):
        gws.graph_watershed_assignments(0, _job_config(tmp_path / 'c', cfg))


def test_assignment_dataset_layout(tmp_path):
    path = str(tmp_path / 'o.n5')
    labels = np.arange(10, dtype='uint64') * np.uint64(2 ** 40)
    cc.write_assignments(path, 'a', labels, (4,))
    ds = File(path)['a']
    assert tuple(ds.shape) == (10,) and tuple(ds.chunks) == (4,) and str(ds.dtype) == 'uint64'
    assert ds.compression == 'gzip'
    np.testing.assert_array_equal(ds[:], labels)
    cc.write_assignments(path, 'a', labels[::-1], (4,))  # a rerun writes into the dataset that is there
    np.testing.assert_array_equal(File(path)['a'][:], labels[::-1])
