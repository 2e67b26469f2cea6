"""CPU restatement of the region adjacency graph of a label block for the tests
(`nrag.gridRag(seg).uvIds()` in test/graph/test_graph.py:63-126; nifty is not available, so this
is a restatement): nodes = np.unique(seg) (without 0 under ignore_label), edges = the sorted set
of (min(u, v), max(u, v)) over all face-adjacent voxel pairs with u != v (none with a 0 under
ignore_label), counts = the voxel pairs per edge."""
import numpy as np


def rag(seg, ignore_label):
    """-> (nodes (n,), edges (m, 2), counts (m,)), uint64; shifted views per axis."""
    seg = np.asarray(seg, dtype=np.uint64)
    assert seg.ndim == 3
    nodes = np.unique(seg)
    if ignore_label:
        nodes = nodes[nodes != 0]
    pairs = []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        u, v = seg[tuple(lo)].ravel(), seg[tuple(hi)].ravel()
        keep = u != v
        if ignore_label:
            keep &= (u != 0) & (v != 0)
        u, v = u[keep], v[keep]
        pairs.append(np.stack([np.minimum(u, v), np.maximum(u, v)], axis=1))
    pairs = np.concatenate(pairs)
    if len(pairs) == 0:
        return nodes, np.zeros((0, 2), np.uint64), np.zeros(0, np.uint64)
    edges, counts = np.unique(pairs, axis=0, return_counts=True)
    return nodes, edges.astype(np.uint64), counts.astype(np.uint64)


def rag_brute(seg, ignore_label):
    """The same by a triple loop over the voxels (tiny arrays only)."""
    seg = np.asarray(seg, dtype=np.uint64)
    nz, ny, nx = seg.shape
    nodes, edges = set(), {}
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                u = int(seg[z, y, x])
                if u != 0 or not ignore_label:
                    nodes.add(u)
                for dz, dy, dx in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
                    zz, yy, xx = z + dz, y + dy, x + dx
                    if zz >= nz or yy >= ny or xx >= nx:
                        continue
                    v = int(seg[zz, yy, xx])
                    if u == v or (ignore_label and (u == 0 or v == 0)):
                        continue
                    e = (min(u, v), max(u, v))
                    edges[e] = edges.get(e, 0) + 1
    keys = sorted(edges)
    return (np.array(sorted(nodes), dtype=np.uint64), np.array(keys, dtype=np.uint64).reshape(-1, 2),
            np.array([edges[k] for k in keys], dtype=np.uint64))


def n_face_pairs(seg, ignore_label):
    """The number of face-adjacent voxel pairs with different, not ignored ids."""
    return int(rag(seg, ignore_label)[2].sum())


def extended_box(blocking, block_id, shape):
    """The box of a block's sub-graph: [begin, min(end + 1, shape)) per axis (increaseRoi=True)."""
    block = blocking.getBlock(block_id)
    return tuple(slice(b, min(e + 1, s)) for b, e, s in zip(block.begin, block.end, shape))


def documented_case():
    """fragments((9, 21, 70)) with [2:5, 3:9, 60:68] = 0: 70 is no multiple of 64, so rows cross
    waves, and the hole straddles lane 63 | 64."""
    from size_filter_ref import fragments
    seg = fragments((9, 21, 70))[0].astype(np.uint64)
    seg[2:5, 3:9, 60:68] = 0
    return seg


def workflow_volume():
    """The workflow tests' volume: fragments((20, 48, 80)) with a zero corner that covers block 0's
    extended box and one label over block 11's (block shape [8, 32, 32])."""
    from size_filter_ref import fragments
    seg = fragments((20, 48, 80))[0].astype(np.uint64)
    seg[0:9, 0:33, 0:33] = 0
    seg[8:17, 32:48, 64:80] = seg.max()
    return seg
