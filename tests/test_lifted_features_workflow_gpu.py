"""LiftedFeaturesFromNodeLabelsWorkflow (target='local') end to end on the GPU on a small n5 volume:
24 x 48 x 80 fragments with maxId, blocks 10 x 32 x 32, 2 jobs.  GraphWorkflow runs once; the lifted
workflow (which runs NodeLabelWorkflow itself) runs with depth 3 for mode 'all', mode 'different'
and once with clear labels.  The lifted edges equal the restatement (tests/lifted_features_ref.py)
applied to the graph's `edges` and the node labels read back, the costs equal the restated rule.
The check that the volume exercises every rule needs no GPU."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import luigi_build

from cluster_tools_amd.utils import volume_utils as vu
import graph_ref as G
import node_labels_ref as NL
import lifted_features_ref as R

SHAPE = (24, 48, 80)
BLOCK_SHAPE = [10, 32, 32]
MAX_ID = 80
DEPTH = 3


def make_volume():
    """Fragments: cells of 6 x 12 x 16 voxels with the ids 1..80; fragment 1 is zeroed (a node
    without a voxel).  Labels: objects of 12 x 24 x 32 voxels with the ids 1..12 on background 0
    that leaves whole fragments unlabelled (x in [16, 32) and the top slab of y in [24, 36)).
    Clear labels: two halves along x, cut at x = 40 through the fragments of x in [32, 48)."""
    z, y, x = np.meshgrid(np.arange(SHAPE[0]), np.arange(SHAPE[1]), np.arange(SHAPE[2]), indexing='ij')
    seg = (1 + (z // 6) * 20 + (y // 12) * 5 + x // 16).astype(np.uint64)
    seg[seg == 1] = 0
    gt = (1 + (z // 12) * 6 + (y // 24) * 3 + x // 32).astype(np.uint64)
    gt[:, :, 16:32] = 0
    gt[0:6, 24:36, :] = 0
    clear = (1 + x // 40).astype(np.uint64)
    clear[:, :, 40:44] = 1  # (no tie in the fragments the cut runs through)
    return seg, gt, clear


def restated(seg, gt, clear):
    """(edges, node labels, clear node labels) of the volume by the restatements alone."""
    _, edges, _ = G.rag(seg, True)
    labels = NL.max_overlap(NL.overlap_rows(seg, gt, 0), MAX_ID + 1, 0)
    clear_labels = NL.max_overlap(NL.overlap_rows(seg, clear, None), MAX_ID + 1, None)
    return edges, labels, clear_labels


def test_the_volume_exercises_every_rule():
    """On the CPU: every mode used gives lifted edges, there are unlabelled nodes, equal and
    unequal label pairs, and the clear labels drop some lifted edges and keep some."""
    edges, labels, clear_labels = restated(*make_volume())
    assert 0 < int((labels == 0).sum()) < MAX_ID and len(np.unique(labels)) > 4
    every = R.lifted_neighborhood(edges, labels, DEPTH, 'all')
    diff = R.lifted_neighborhood(edges, labels, DEPTH, 'different')
    assert 0 < len(diff) < len(every)
    kept = R.clear_lifted_edges(every, clear_labels)
    assert 0 < len(kept) < len(every)
    costs = R.lifted_costs(every, labels)
    assert (costs == 6).any() and (costs == -6).any()


@pytest.fixture(scope='module')
def problem(tmp_path_factory):
    """The volume as n5, the configs, and the graph (GraphWorkflow, once for the module)."""
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    from cluster_tools_amd.graph import GraphWorkflow
    root = tmp_path_factory.mktemp('lifted')
    seg, gt, clear = make_volume()
    cfg_dir = root / 'configs'
    cfg_dir.mkdir()
    g = BaseClusterTask.default_global_config()
    g['shebang'] = '#! ' + sys.executable
    g['block_shape'] = BLOCK_SHAPE
    (cfg_dir / 'global.config').write_text(json.dumps(g))
    path = str(root / 'data.n5')
    with vu.file_reader(path) as f:
        ds = f.create_dataset('seg', data=seg, chunks=(8, 16, 16))
        ds.attrs['maxId'] = MAX_ID
        f.create_dataset('gt', data=gt, chunks=(8, 16, 16))
        f.create_dataset('clear', data=clear, chunks=(8, 16, 16))
    graph_path, tmp_folder = str(root / 'graph.n5'), str(root / 'tmp_graph')
    luigi_build(GraphWorkflow(tmp_folder=tmp_folder, config_dir=str(cfg_dir), max_jobs=2, target='local',
                              input_path=path, input_key='seg', graph_path=graph_path, output_key='graph'),
                tmp_folder)
    with vu.file_reader(graph_path, 'r') as f:
        edges = f['graph/edges'][:]
    np.testing.assert_array_equal(edges, restated(seg, gt, clear)[0])
    return dict(root=root, cfg_dir=str(cfg_dir), path=path, graph_path=graph_path, edges=edges)


def _run(problem, name, **kwargs):
    from cluster_tools_amd.lifted_features import LiftedFeaturesFromNodeLabelsWorkflow
    out_path, tmp_folder = str(problem['root'] / ('out_%s.n5' % name)), str(problem['root'] / ('tmp_%s' % name))
    task = LiftedFeaturesFromNodeLabelsWorkflow(
        tmp_folder=tmp_folder, config_dir=problem['cfg_dir'], max_jobs=2, target='local', ws_path=problem['path'],
        ws_key='seg', labels_path=problem['path'], labels_key='gt', graph_path=problem['graph_path'],
        graph_key='graph', output_path=out_path, nh_out_key='lifted_nh', feat_out_key='lifted_costs', prefix='nuc',
        nh_graph_depth=DEPTH, label_ignore_label=0, **kwargs)
    luigi_build(task, tmp_folder)
    return out_path, tmp_folder


def _check(problem, out_path, tmp_folder, mode, with_clear):
    seg, gt, clear = make_volume()
    _, want_labels, want_clear = restated(seg, gt, clear)
    with vu.file_reader(out_path, 'r') as f:
        labels = f['node_overlaps/nuc'][:]
        np.testing.assert_array_equal(labels, want_labels)
        searched = R.lifted_neighborhood(problem['edges'], labels, DEPTH, mode)
        want = searched
        if with_clear:
            clear_labels = f['node_overlaps/clear_nuc'][:]
            np.testing.assert_array_equal(clear_labels, want_clear)
            want = R.clear_lifted_edges(searched, clear_labels)
            assert 0 < len(want) < len(searched)
        k = len(want)
        assert k > 0
        ds = f['lifted_nh']
        assert tuple(ds.shape) == (k, 2) and tuple(ds.chunks) == (min(k, 262144), 2) and str(ds.dtype) == 'uint64'
        lifted = ds[:]
        np.testing.assert_array_equal(lifted, want)
        ds = f['lifted_costs']
        assert tuple(ds.shape) == (k,) and tuple(ds.chunks) == (min(k, 262144),) and str(ds.dtype) == 'float32'
        np.testing.assert_array_equal(ds[:], R.lifted_costs(want, labels))
    log = open(os.path.join(tmp_folder, 'logs', 'sparse_lifted_neighborhood_nuc_0.log')).read()
    assert 'extracted %i lifted edges' % len(searched) in log
    assert 'lifted nh mode set to %s, depth set to %i' % (mode, DEPTH) in log
    for name in ('sparse_lifted_neighborhood_nuc.log', 'costs_from_node_labels_nuc.log',
                 'sparse_lifted_neighborhood_job_nuc_0.config', 'costs_from_node_labels_job_nuc_0.config'):
        assert os.path.exists(os.path.join(tmp_folder, name)), name
    return lifted


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['all', 'different'])
def test_lifted_features(problem, mode):
    out_path, tmp_folder = _run(problem, mode, mode=mode)
    lifted = _check(problem, out_path, tmp_folder, mode, False)
    assert not os.path.exists(os.path.join(tmp_folder, 'clear_lifted_edges_from_labels.log'))
    # no lifted edge is a graph edge
    both = np.concatenate([lifted, problem['edges']])
    assert len(np.unique(both, axis=0)) == len(both)


@pytest.mark.gpu
def test_lifted_features_with_clear_labels(problem):
    out_path, tmp_folder = _run(problem, 'clear', clear_labels_path=problem['path'], clear_labels_key='clear')
    _check(problem, out_path, tmp_folder, 'all', True)
    log = open(os.path.join(tmp_folder, 'logs', 'clear_lifted_edges_from_labels_0.log')).read()
    assert 'clear number of lifted edges from' in log
