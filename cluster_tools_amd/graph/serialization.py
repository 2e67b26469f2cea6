"""The on-disk layout of a graph group, as the reference's Python readers and writers use it
(multicut/reduce_problem.py:259-285, 310-332, multicut/solve_global.py:124-133,
learning/edge_labels.py:112, stitching/simple_stitch_edges.py:47, test/graph/test_graph.py:83-86):
attributes numberOfNodes, numberOfEdges, ignoreLabel (block groups: roiBegin, roiEnd; the final
graph: shape), datasets `nodes` (n,) and `edges` (m, 2), uint64, gzip.  A table of length 0 is
not written as a dataset: the attributes say 0 and the readers here return an empty table."""
import numpy as np

CHUNK = 262144  # rows per chunk (reduce_problem.py:269-275)


def write_graph(f, key, nodes, edges, ignore_label, **attrs):
    nodes = np.ascontiguousarray(nodes, dtype='uint64')
    edges = np.ascontiguousarray(edges, dtype='uint64').reshape(-1, 2)
    if key in f:  # a retried block: no stale table may survive
        del f[key]
    g = f.require_group(key)
    n, m = len(nodes), len(edges)
    if n:
        g.create_dataset('nodes', data=nodes, chunks=(min(n, CHUNK),), compression='gzip')
    if m:
        g.create_dataset('edges', data=edges, chunks=(min(m, CHUNK), 2), compression='gzip')
    for k, v in dict(attrs, numberOfNodes=n, numberOfEdges=m, ignoreLabel=bool(ignore_label)).items():
        g.attrs[k] = v
    return g


def read_table(g, name, width=None):
    """A dataset of a graph group, or the empty table when it was not written."""
    if name in g:
        return g[name][:]
    return np.zeros((0,) if width is None else (0, width), dtype='uint64')


def read_graph(f, key):
    g = f[key]
    return read_table(g, 'nodes'), read_table(g, 'edges', 2)


def write_edge_ids(f, key, edge_ids):
    g = f[key]
    if 'edgeIds' in g:
        del g['edgeIds']
    m = len(edge_ids)
    if m:
        g.create_dataset('edgeIds', data=np.ascontiguousarray(edge_ids, dtype='uint64'), chunks=(min(m, CHUNK),),
                         compression='gzip')
