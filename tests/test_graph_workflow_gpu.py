"""GraphWorkflow (target='local') end to end on the GPU, on a small n5 volume with 18 blocks,
ragged on every axis: every block's sub-graph against the CPU restatement (tests/graph_ref.py) on
its extended box, the final graph against the restatement on the whole volume, the attributes and
the edge id mapping; two scales, a global roi and ids above 2^32."""
import json
import sys

import numpy as np
import pytest

from conftest import luigi_build

from cluster_tools_amd.utils import volume_utils as vu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.graph.serialization import read_graph, read_table
import graph_ref as G

pytestmark = pytest.mark.gpu

SHAPE = (20, 48, 80)
BLOCK_SHAPE = [8, 32, 32]
N_BLOCKS = 18
SHIFT = np.uint64(2 ** 33)


class _Volume:
    def __init__(self):
        self.seg = G.workflow_volume()
        assert self.seg.shape == SHAPE
        self.blocking = Blocking([0, 0, 0], list(SHAPE), BLOCK_SHAPE)
        assert self.blocking.numberOfBlocks == N_BLOCKS
        self.whole = {ign: G.rag(self.seg, ign) for ign in (False, True)}
        assert [len(t) for t in self.whole[False][:2]] == [49, 181]
        assert [len(t) for t in self.whole[True][:2]] == [48, 167]
        # block 0's extended box is all 0, block 11's a single label
        assert not self.seg[G.extended_box(self.blocking, 0, SHAPE)].any()
        assert len(np.unique(self.seg[G.extended_box(self.blocking, 11, SHAPE)])) == 1


@pytest.fixture(scope='module')
def volume():
    return _Volume()


def _run(tmp_path, seg, ignore_label=True, n_scales=1, roi=None):
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    from cluster_tools_amd.graph import GraphWorkflow
    cfg_dir = tmp_path / 'configs'
    cfg_dir.mkdir()
    g = BaseClusterTask.default_global_config()
    g['shebang'] = '#! ' + sys.executable
    g['block_shape'] = BLOCK_SHAPE
    if roi is not None:
        g['roi_begin'], g['roi_end'] = roi
    (cfg_dir / 'global.config').write_text(json.dumps(g))
    cfg = GraphWorkflow.get_config()['initial_sub_graphs']
    cfg['ignore_label'] = ignore_label
    (cfg_dir / 'initial_sub_graphs.config').write_text(json.dumps(cfg))
    path = str(tmp_path / 'data.n5')
    with vu.file_reader(path) as f:
        f.create_dataset('seg', data=seg, chunks=(8, 16, 16))
    graph_path = str(tmp_path / 'graph.n5')
    tmp_folder = str(tmp_path / 'tmp')
    task = GraphWorkflow(tmp_folder=tmp_folder, config_dir=str(cfg_dir), max_jobs=2, target='local',
                         input_path=path, input_key='seg', graph_path=graph_path, output_key='graph',
                         n_scales=n_scales)
    luigi_build(task, tmp_folder)
    return graph_path


def _check_graph_group(g, ref, ignore_label):
    nodes, edges = read_table(g, 'nodes'), read_table(g, 'edges', 2)
    np.testing.assert_array_equal(nodes, ref[0])
    np.testing.assert_array_equal(edges, ref[1])
    assert g.attrs['numberOfNodes'] == len(ref[0]) and g.attrs['numberOfEdges'] == len(ref[1])
    assert g.attrs['ignoreLabel'] is bool(ignore_label)
    # empty tables are not written
    assert ('nodes' in g) == (len(ref[0]) > 0) and ('edges' in g) == (len(ref[1]) > 0)
    return edges


def _check_blocks(f, seg, scale, block_ids, ignore_label, global_edges):
    blocking = Blocking([0, 0, 0], list(SHAPE), [2 ** scale * b for b in BLOCK_SHAPE])
    for block_id in block_ids:
        g = f['s%i/sub_graphs/block_%i' % (scale, block_id)]
        bb = G.extended_box(blocking, block_id, SHAPE)
        assert g.attrs['roiBegin'] == [s.start for s in bb] and g.attrs['roiEnd'] == [s.stop for s in bb]
        edges = _check_graph_group(g, G.rag(seg[bb], ignore_label), ignore_label)
        edge_ids = read_table(g, 'edgeIds')
        assert edge_ids.dtype == np.uint64 and edge_ids.shape == (len(edges),)
        assert ('edgeIds' in g) == (len(edges) > 0)
        np.testing.assert_array_equal(global_edges[edge_ids.astype(np.int64)], edges)


@pytest.mark.parametrize('ignore_label', [True, False])
def test_graph_workflow(tmp_path, volume, ignore_label):
    graph_path = _run(tmp_path, volume.seg, ignore_label)
    with vu.file_reader(graph_path, 'r') as f:
        assert list(f.attrs['shape']) == list(SHAPE)
        final = f['graph']
        assert list(final.attrs['shape']) == list(SHAPE)
        global_edges = _check_graph_group(final, volume.whole[ignore_label], ignore_label)
        _check_blocks(f, volume.seg, 0, range(N_BLOCKS), ignore_label, global_edges)
        empty = f['s0/sub_graphs/block_0']
        if ignore_label:
            assert empty.attrs['numberOfNodes'] == 0 and 'nodes' not in empty
        else:
            assert read_table(empty, 'nodes').tolist() == [0]
        assert f['s0/sub_graphs/block_11'].attrs['numberOfNodes'] == 1
        assert f['s0/sub_graphs/block_11'].attrs['numberOfEdges'] == 0


def test_two_scales(tmp_path, volume):
    graph_path = _run(tmp_path, volume.seg, True, n_scales=2)
    with vu.file_reader(graph_path, 'r') as f:
        global_edges = _check_graph_group(f['graph'], volume.whole[True], True)
        _check_blocks(f, volume.seg, 0, range(N_BLOCKS), True, global_edges)
        n1 = Blocking([0, 0, 0], list(SHAPE), [2 * b for b in BLOCK_SHAPE]).numberOfBlocks
        assert n1 == 4 and sorted(f['s1/sub_graphs'].keys()) == sorted('block_%i' % b for b in range(n1))
        _check_blocks(f, volume.seg, 1, range(n1), True, global_edges)


def test_global_roi(tmp_path, volume):
    # z 8:20, every y, x 32:80 -> the blocks 7-8, 10-11, 13-14, 16-17
    graph_path = _run(tmp_path, volume.seg, True, roi=([8, 0, 32], [20, 48, 80]))
    blocks = [7, 8, 10, 11, 13, 14, 16, 17]
    with vu.file_reader(graph_path, 'r') as f:
        assert sorted(f['s0/sub_graphs'].keys()) == sorted('block_%i' % b for b in blocks)
        nodes, edges = read_graph(f, 'graph')
        ref = G.rag(volume.seg[8:20, 0:48, 32:80], True)
        np.testing.assert_array_equal(nodes, ref[0])
        np.testing.assert_array_equal(edges, ref[1])
        _check_blocks(f, volume.seg, 0, blocks, True, edges)


def test_large_ids(tmp_path, volume):
    big = np.where(volume.seg != 0, volume.seg + SHIFT, np.uint64(0))
    graph_path = _run(tmp_path, big, True)
    with vu.file_reader(graph_path, 'r') as f:
        nodes, edges = read_graph(f, 'graph')
        np.testing.assert_array_equal(nodes, volume.whole[True][0] + SHIFT)
        np.testing.assert_array_equal(edges, volume.whole[True][1] + SHIFT)
        _check_blocks(f, big, 0, range(N_BLOCKS), True, edges)
