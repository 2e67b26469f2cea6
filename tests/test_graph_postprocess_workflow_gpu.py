"""ConnectedComponentsWorkflow and SizeFilterAndGraphWatershedWorkflow (target='local') end to end
on the GPU, on the small n5 volume of the graph workflow tests (20 x 48 x 80 fragments, blocks
8 x 32 x 32).  GraphWorkflow and EdgeFeaturesWorkflow run once for the module and write the graph and
the merged features into one container (the `problem_path` of the reference).  The assignments the
workflows write equal the restatement (tests/graph_postprocess_ref.py) applied to the graph, the
features, the assignments and the discard ids read back from disk; the volumes the Write step makes
equal the assignments looked up at the fragments (Write skips a block without a fragment: such a
block stays 0, write.py)."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import luigi_build

from cluster_tools_amd.utils import volume_utils as vu
from cluster_tools_amd.utils.blocking import Blocking
import graph_ref as G
import graph_postprocess_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (20, 48, 80)
BLOCK_SHAPE = [8, 32, 32]
SIZE_THRESHOLD = 500


@pytest.fixture(scope='module')
def problem(tmp_path_factory):
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    from cluster_tools_amd.graph import GraphWorkflow
    from cluster_tools_amd.features import EdgeFeaturesWorkflow
    root = tmp_path_factory.mktemp('graph_postprocess')
    seg = G.workflow_volume()
    assert seg.shape == SHAPE
    bmap = np.random.default_rng(0).random(SHAPE, dtype=np.float32)
    cfg_dir = root / 'configs'
    cfg_dir.mkdir()
    g = BaseClusterTask.default_global_config()
    g['shebang'] = '#! ' + sys.executable
    g['block_shape'] = BLOCK_SHAPE
    (cfg_dir / 'global.config').write_text(json.dumps(g))
    path, problem_path, tmp_folder = str(root / 'data.n5'), str(root / 'problem.n5'), str(root / 'tmp_problem')
    with vu.file_reader(path) as f:
        f.create_dataset('seg', data=seg, chunks=(8, 16, 16))
        f.create_dataset('bmap', data=bmap, chunks=(8, 16, 16))
    common = dict(tmp_folder=tmp_folder, config_dir=str(cfg_dir), target='local')
    graph = GraphWorkflow(max_jobs=2, input_path=path, input_key='seg', graph_path=problem_path, output_key='graph',
                          **common)
    luigi_build(EdgeFeaturesWorkflow(max_jobs=2, max_jobs_merge=1, input_path=path, input_key='bmap', labels_path=path,
                                     labels_key='seg', graph_path=problem_path, graph_key='graph',
                                     output_path=problem_path, output_key='features', dependency=graph, **common),
                tmp_folder)
    with vu.file_reader(problem_path, 'r') as f:
        edges, features = f['graph/edges'][:], f['features'][:]
    assert features.shape == (len(edges), 10)
    n_nodes = int(edges.max()) + 1
    assert n_nodes == int(seg.max()) + 1
    ids = np.arange(n_nodes)
    ass7 = (1 + ids % 7).astype('uint64')
    ass23 = (1 + ids % 23).astype('uint64')
    ass23[0] = 0
    with vu.file_reader(path) as f:
        f.create_dataset('ass7', data=ass7, chunks=(16,))
        f.create_dataset('ass23', data=ass23, chunks=(16,))
        f.create_dataset('seg23', data=ass23[seg], chunks=(8, 16, 16))  # the segmentation written from ass23
    return dict(root=root, cfg_dir=str(cfg_dir), path=path, problem_path=problem_path, seg=seg, edges=edges,
                features=features, ass7=ass7, ass23=ass23)


def _written(seg, assignments):
    """assignments[seg], and 0 in the blocks without a fragment, which Write leaves alone."""
    want = assignments[seg]
    blocking = Blocking([0, 0, 0], list(SHAPE), BLOCK_SHAPE)
    skipped = []
    for block_id in range(blocking.numberOfBlocks):
        bb = vu.block_to_bb(blocking.getBlock(block_id))
        if not seg[bb].any():
            want[bb] = 0
            skipped.append(block_id)
    return want, skipped


def _check_assignment_dataset(f, key, want):
    ds = f[key]
    assert tuple(ds.shape) == (len(want),) and tuple(ds.chunks) == (16,) and str(ds.dtype) == 'uint64'
    assert ds.compression == 'gzip'
    got = ds[:]
    np.testing.assert_array_equal(got, want)
    return got


def test_connected_components_workflow(problem):
    from cluster_tools_amd.postprocess import ConnectedComponentsWorkflow
    out_path, tmp_folder = str(problem['root'] / 'out_cc.n5'), str(problem['root'] / 'tmp_cc')
    luigi_build(ConnectedComponentsWorkflow(
        tmp_folder=tmp_folder, config_dir=problem['cfg_dir'], max_jobs=2, target='local',
        problem_path=problem['problem_path'], graph_key='graph', path=problem['path'], fragments_key='seg',
        assignment_path=problem['path'], assignment_key='ass7', output_path=out_path, assignment_out_key='cc',
        output_key='cc_seg'), tmp_folder)
    want = R.components(problem['edges'], problem['ass7'])
    assert want.max() > 7  # the segments are not connected: there is something to split
    with vu.file_reader(out_path, 'r') as f:
        got = _check_assignment_dataset(f, 'cc', want)
        volume, skipped = _written(problem['seg'], got)
        assert skipped == [0]
        np.testing.assert_array_equal(f['cc_seg'][:], volume)
    for name in ('graph_connected_components.log', 'graph_connected_components_job_0.config',
                 'write_graph-connected-components.log'):
        assert os.path.exists(os.path.join(tmp_folder, name)), name
    assert 'processed job 0' in open(os.path.join(tmp_folder, 'logs', 'graph_connected_components_0.log')).read()


@pytest.mark.parametrize('relabel,from_costs', [(False, False), (False, True), (True, False), (True, True)])
def test_size_filter_and_graph_watershed_workflow(problem, relabel, from_costs):
    from cluster_tools_amd.postprocess import SizeFilterAndGraphWatershedWorkflow
    name = 'gws_%i%i' % (relabel, from_costs)
    out_path, tmp_folder = str(problem['root'] / ('out_%s.n5' % name)), str(problem['root'] / ('tmp_%s' % name))
    with_write = relabel and not from_costs  # (the Write step once)
    luigi_build(SizeFilterAndGraphWatershedWorkflow(
        tmp_folder=tmp_folder, config_dir=problem['cfg_dir'], max_jobs=1, target='local',
        problem_path=problem['problem_path'], graph_key='graph', features_key='features', path=problem['path'],
        segmentation_key='seg23', fragments_key='seg', assignment_key='ass23', size_threshold=SIZE_THRESHOLD,
        relabel=relabel, from_costs=from_costs, output_path=out_path, assignment_out_key='gws',
        output_key='gws_seg' if with_write else ''), tmp_folder)
    edges, ass = problem['edges'], problem['ass23']
    discard_ids = np.load(os.path.join(tmp_folder, 'discard_ids.npy'))
    assert len(discard_ids) > 0 and 0 not in discard_ids
    sizes = np.bincount(ass[problem['seg']].ravel().astype(np.int64))
    np.testing.assert_array_equal(discard_ids, np.nonzero((sizes > 0) & (sizes < SIZE_THRESHOLD))[0])
    want = R.task_result(edges, problem['features'][:, 0], ass, discard_ids, relabel, from_costs)
    with vu.file_reader(out_path, 'r') as f:
        got = _check_assignment_dataset(f, 'gws', want)
        if with_write:
            volume, skipped = _written(problem['seg'], got)
            assert skipped == [0]
            np.testing.assert_array_equal(f['gws_seg'][:], volume)
        else:
            assert 'gws_seg' not in f
    # no discarded id survives among the nodes a seed can reach
    seeds, seed_offset = R.task_seeds(ass, discard_ids)
    parts = R.components(edges, np.ones(len(ass), dtype='uint64'))
    reached = np.isin(parts, parts[seeds != 0])
    assert reached.sum() > (seeds != 0).sum() and (seeds[reached] == 0).any()
    plain = R.task_result(edges, problem['features'][:, 0], ass, discard_ids, False, from_costs)
    assert not np.isin(plain[reached], discard_ids).any()
    if not relabel:
        assert not np.isin(got[reached], discard_ids).any()
        np.testing.assert_array_equal(got[seeds != 0], np.where(ass == 0, 0, ass)[seeds != 0])  # kept segments stay
    else:
        assert got.max() == len(np.unique(plain[plain != 0]))
    log = open(os.path.join(tmp_folder, 'logs', 'graph_watershed_assignments_0.log')).read()
    for line in ('Read features and edges from %s' % problem['problem_path'], 'Read assignments from %s' % problem['path'],
                 'Discarding %i fragments' % int(np.isin(ass, discard_ids).sum()), 'Start grah watershed',
                 'Finished graph watershed', 'processed job 0'):
        assert line in log, line
    assert ('Mapping costs with range' in log) == from_costs
