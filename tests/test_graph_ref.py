"""CPU checks of the graph path: the numpy restatement of the region adjacency graph
(tests/graph_ref.py) against a triple-loop brute force, the task surface of GraphWorkflow, and
MapEdgeIds' id mapping on hand-made tables.  No GPU."""
import numpy as np
import pytest

import graph_ref as G


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype == np.uint64 and x.shape == y.shape, (x.shape, y.shape)
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize('ignore_label', [False, True])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_restatement_equals_brute_force_random(seed, ignore_label):
    seg = np.random.RandomState(seed).randint(0, 5, (4, 5, 6)).astype(np.uint64)
    assert (seg == 0).any()
    _same(G.rag(seg, ignore_label), G.rag_brute(seg, ignore_label))


@pytest.mark.parametrize('ignore_label,n_nodes,n_edges,n_pairs', [(False, 25, 82, 4152), (True, 24, 80, 3972)])
def test_restatement_equals_brute_force_documented(ignore_label, n_nodes, n_edges, n_pairs):
    seg = G.documented_case()
    nodes, edges, counts = G.rag(seg, ignore_label)
    assert (len(nodes), len(edges), int(counts.sum())) == (n_nodes, n_edges, n_pairs)
    _same((nodes, edges, counts), G.rag_brute(seg, ignore_label))


def test_restatement_arange_and_degenerate():
    seg = (np.arange(5 * 6 * 67).reshape(5, 6, 67) + 1).astype(np.uint64)
    nodes, edges, counts = G.rag(seg, True)
    assert len(nodes) == seg.size and len(edges) == 5263 and (counts == 1).all()
    _same((nodes, edges, counts), G.rag_brute(seg, True))
    const = np.full((2, 3, 4), 7, np.uint64)
    assert [len(t) for t in G.rag(const, True)] == [1, 0, 0]
    zero = np.zeros((2, 3, 4), np.uint64)
    assert [len(t) for t in G.rag(zero, True)] == [0, 0, 0]
    assert G.rag(zero, False)[0].tolist() == [0] and G.rag(zero, False)[1].shape == (0, 2)


def test_workflow_volume_figures():
    seg = G.workflow_volume()
    assert [len(t) for t in G.rag(seg, False)[:2]] == [49, 181]
    assert [len(t) for t in G.rag(seg, True)[:2]] == [48, 167]


def test_task_surface():
    from cluster_tools_amd.graph import GraphWorkflow
    from cluster_tools_amd.graph import initial_sub_graphs, merge_sub_graphs, map_edge_ids
    for mod, base in ((initial_sub_graphs, 'InitialSubGraphs'), (merge_sub_graphs, 'MergeSubGraphs'),
                      (map_edge_ids, 'MapEdgeIds')):
        for target in ('Local', 'Slurm', 'LSF'):
            assert hasattr(mod, base + target)
    assert initial_sub_graphs.InitialSubGraphsBase.task_name == 'initial_sub_graphs'
    assert merge_sub_graphs.MergeSubGraphsBase.task_name == 'merge_sub_graphs'
    assert map_edge_ids.MapEdgeIdsBase.task_name == 'map_edge_ids'
    cfg = initial_sub_graphs.InitialSubGraphsLocal.default_task_config()
    assert cfg['ignore_label'] is True and cfg['threads_per_job'] == 1
    config = GraphWorkflow.get_config()
    assert {'global', 'initial_sub_graphs', 'merge_sub_graphs', 'map_edge_ids'} <= set(config)


def test_task_logs(tmp_path):
    from cluster_tools_amd.graph.merge_sub_graphs import MergeSubGraphsLocal
    from cluster_tools_amd.graph.map_edge_ids import MapEdgeIdsLocal
    from cluster_tools_amd.utils.task_utils import DummyTask
    kw = dict(tmp_folder=str(tmp_path), max_jobs=1, config_dir=str(tmp_path), graph_path='g.n5', dependency=DummyTask())
    final = MergeSubGraphsLocal(scale=1, merge_complete_graph=True, output_key='graph', **kw)
    blocks = MergeSubGraphsLocal(scale=1, **kw)
    assert final.output().path.endswith('merge_sub_graphs_s1.log')
    # the two merges GraphWorkflow runs at the last scale must not share a target
    assert blocks.output().path != final.output().path
    assert MapEdgeIdsLocal(scale=2, input_key='graph', **kw).output().path.endswith('map_edge_ids_s2.log')


def test_workflow_refuses_h5(tmp_path):
    from cluster_tools_amd.graph import GraphWorkflow
    task = GraphWorkflow(tmp_folder=str(tmp_path), max_jobs=1, config_dir=str(tmp_path), target='local',
                         input_path='seg.h5', input_key='seg', graph_path='graph.n5', output_key='graph')
    with pytest.raises(AssertionError, match='n5 and zarr'):
        task.requires()


def test_workflow_maps_every_scale(tmp_path):
    from cluster_tools_amd.graph import GraphWorkflow
    task = GraphWorkflow(tmp_folder=str(tmp_path), max_jobs=1, config_dir=str(tmp_path), target='local',
                         input_path='seg.n5', input_key='seg', graph_path='graph.n5', output_key='graph', n_scales=3)
    chain, dep = [], task.requires()
    while hasattr(dep, 'task_name'):
        chain.append((dep.task_name, getattr(dep, 'scale', None), getattr(dep, 'merge_complete_graph', None)))
        dep = dep.dependency
    assert chain[::-1] == [('initial_sub_graphs', None, None), ('merge_sub_graphs', 1, False),
                           ('merge_sub_graphs', 2, False), ('merge_sub_graphs', 2, True),
                           ('map_edge_ids', 0, None), ('map_edge_ids', 1, None), ('map_edge_ids', 2, None)]


def test_edge_id_mapping():
    from cluster_tools_amd.graph.map_edge_ids import EdgeIndex
    big = 2 ** 64 - 1
    global_edges = np.array([[1, 2], [1, 7], [2, 3], [2, 2 ** 33], [3, 7], [7, big], [2 ** 33, big]], dtype=np.uint64)
    index = EdgeIndex(global_edges)
    block = np.array([[2, 3], [7, big], [1, 2], [2 ** 33, big]], dtype=np.uint64)
    ids = index.edge_ids(block)
    assert ids.dtype == np.uint64 and ids.tolist() == [2, 5, 0, 6]
    np.testing.assert_array_equal(global_edges[ids], block)
    np.testing.assert_array_equal(index.edge_ids(global_edges), np.arange(7, dtype=np.uint64))
    # an empty block
    empty = index.edge_ids(np.zeros((0, 2), np.uint64))
    assert empty.shape == (0,) and empty.dtype == np.uint64
    # an edge between known nodes that is no global edge, and an unknown node
    for bad in ([[1, 3]], [[1, 5]], [[2 ** 33, 2 ** 34]]):
        with pytest.raises(RuntimeError, match='not in the global graph'):
            index.edge_ids(np.array(bad, dtype=np.uint64))


def test_graph_serialization_roundtrip(tmp_path):
    from cluster_tools_amd.utils import volume_utils as vu
    from cluster_tools_amd.graph.serialization import write_graph, read_graph, write_edge_ids, read_table
    nodes = np.array([1, 2 ** 33, 2 ** 64 - 1], dtype=np.uint64)
    edges = np.array([[1, 2 ** 33], [2 ** 33, 2 ** 64 - 1]], dtype=np.uint64)
    with vu.file_reader(str(tmp_path / 'g.n5')) as f:
        write_graph(f, 's0/sub_graphs/block_3', nodes, edges, True, roiBegin=[0, 1, 2], roiEnd=[3, 4, 5])
        write_graph(f, 's0/sub_graphs/block_4', nodes[:0], edges[:0], False)
        g = f['s0/sub_graphs/block_3']
        assert (g.attrs['numberOfNodes'], g.attrs['numberOfEdges'], g.attrs['ignoreLabel']) == (3, 2, True)
        assert g.attrs['roiBegin'] == [0, 1, 2] and g.attrs['roiEnd'] == [3, 4, 5]
        assert g['nodes'].chunks == (3,) and g['edges'].chunks == (2, 2) and g['edges'].dtype == np.uint64
        _same(read_graph(f, 's0/sub_graphs/block_3'), (nodes, edges))
        # empty tables are not written as datasets; the readers give empty tables
        e = f['s0/sub_graphs/block_4']
        assert 'nodes' not in e and 'edges' not in e
        assert (e.attrs['numberOfNodes'], e.attrs['numberOfEdges'], e.attrs['ignoreLabel']) == (0, 0, False)
        _same(read_graph(f, 's0/sub_graphs/block_4'), (nodes[:0], edges[:0]))
        write_edge_ids(f, 's0/sub_graphs/block_3', np.array([4, 9], np.uint64))
        write_edge_ids(f, 's0/sub_graphs/block_4', np.zeros(0, np.uint64))
        assert read_table(g, 'edgeIds').tolist() == [4, 9] and 'edgeIds' not in e
        # a rewritten group keeps nothing of its former tables
        write_graph(f, 's0/sub_graphs/block_3', nodes[:1], edges[:0], True)
        assert 'edges' not in f['s0/sub_graphs/block_3'] and 'edgeIds' not in f['s0/sub_graphs/block_3']
