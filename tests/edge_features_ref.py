"""CPU restatement of the boundary-map edge features for the tests (DESIGN.md section 3.5;
`ndist.extractBlockFeaturesFromBoundaryMaps_*` and `ndist.mergeFeatureBlocks` are not available,
so this is a restatement, as graph_ref.py is one of gridRag).

A block has an extended box (labels, data) and a core extent: a face-adjacent voxel pair
(p, p + e) is owned when p lies in the core, p + e in the extended box, the ids differ and, under
ignore_label, neither is 0.  Both voxel values are samples of the pair's edge.  Row of an edge =
[mean, variance, min, q10, q25, q50, q75, q90, max, count] over its sorted float64 samples."""
import numpy as np

QUANTILES = (0.1, 0.25, 0.5, 0.75, 0.9)
N_FEATS = 10


def to_float32(data):
    """The sample values of a boundary map: float32 as is, uint8 / 255."""
    data = np.asarray(data)
    if data.dtype == np.uint8:
        return data.astype(np.float32) / np.float32(255)
    assert data.dtype == np.float32, data.dtype
    return data


def row_of(samples, count):
    """The ten features of one edge from its samples (any order) and its number of pairs."""
    if count == 0:
        return np.zeros(N_FEATS)
    s = np.sort(np.asarray(samples, dtype=np.float64))
    n = len(s)
    assert n == 2 * count
    mean = s.sum() / n
    var = ((s - mean) ** 2).sum() / n
    row = [mean, var, s[0]]
    for q in QUANTILES:
        pos = q * (n - 1)
        lo = int(np.floor(pos))
        hi = min(lo + 1, n - 1)
        row.append(s[lo] + (pos - lo) * (s[hi] - s[lo]))
    return np.array(row + [s[n - 1], float(count)])


def _edge_index(edges, u, v):
    """Index of every pair (u, v) in the sorted edge table, -1 where it is not in it."""
    edges = np.asarray(edges, dtype=np.uint64).reshape(-1, 2)
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    if len(edges) == 0:
        return np.full(len(lo), -1, dtype=np.int64)
    # ranks over every id in play keep the lexicographic order in one uint64 key
    ids = np.unique(np.concatenate([edges.ravel(), lo, hi]))
    n = np.uint64(len(ids))
    ekeys = np.searchsorted(ids, edges[:, 0]).astype(np.uint64) * n + np.searchsorted(ids, edges[:, 1]).astype(np.uint64)
    assert np.all(ekeys[1:] > ekeys[:-1]), "the edges are not sorted and unique"
    keys = np.searchsorted(ids, lo).astype(np.uint64) * n + np.searchsorted(ids, hi).astype(np.uint64)
    idx = np.searchsorted(ekeys, keys)
    idx[idx == len(ekeys)] = 0
    return np.where(ekeys[idx] == keys, idx, -1).astype(np.int64)


def block_features(labels, data, edges, ignore_label, core_shape=None):
    """-> (features (m, 10) float64 in the order of `edges`, n_missing): shifted views per axis."""
    labels = np.asarray(labels, dtype=np.uint64)
    data = to_float32(data)
    assert labels.ndim == 3 and labels.shape == data.shape
    core = tuple(labels.shape if core_shape is None else core_shape)
    edges = np.asarray(edges, dtype=np.uint64).reshape(-1, 2)
    own = tuple(slice(0, c) for c in core)
    eidx, vals = [], []
    for axis in range(3):
        lo, hi = list(own), [slice(0, c) for c in core]
        stop = min(core[axis], labels.shape[axis] - 1)  # p + e stays in the extended box
        lo[axis], hi[axis] = slice(0, stop), slice(1, stop + 1)
        u, v = labels[tuple(lo)].ravel(), labels[tuple(hi)].ravel()
        keep = u != v
        if ignore_label:
            keep &= (u != 0) & (v != 0)
        eidx.append(_edge_index(edges, u[keep], v[keep]))
        vals.append(np.stack([data[tuple(lo)].ravel()[keep], data[tuple(hi)].ravel()[keep]], axis=1))
    eidx, vals = np.concatenate(eidx), np.concatenate(vals).astype(np.float64)
    n_missing = int((eidx < 0).sum())
    vals, eidx = vals[eidx >= 0], eidx[eidx >= 0]
    order = np.argsort(eidx, kind='stable')
    eidx, vals = eidx[order], vals[order]
    starts = np.searchsorted(eidx, np.arange(len(edges) + 1))
    out = np.zeros((len(edges), N_FEATS))
    for e in range(len(edges)):
        a, b = starts[e], starts[e + 1]
        out[e] = row_of(vals[a:b].ravel(), b - a)
    return out, n_missing


def block_features_brute(labels, data, edges, ignore_label, core_shape=None):
    """The same by a triple loop over the voxels (arrays of at most 5 x 6 x 7)."""
    labels = np.asarray(labels, dtype=np.uint64)
    data = to_float32(data)
    assert labels.size <= 5 * 6 * 7
    nz, ny, nx = labels.shape
    cz, cy, cx = labels.shape if core_shape is None else core_shape
    table = {(int(u), int(v)): i for i, (u, v) in enumerate(np.asarray(edges).reshape(-1, 2))}
    samples = [[] for _ in table]
    n_missing = 0
    for z in range(cz):
        for y in range(cy):
            for x in range(cx):
                u = int(labels[z, y, x])
                for dz, dy, dx in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
                    zz, yy, xx = z + dz, y + dy, x + dx
                    if zz >= nz or yy >= ny or xx >= nx:
                        continue
                    v = int(labels[zz, yy, xx])
                    if u == v or (ignore_label and (u == 0 or v == 0)):
                        continue
                    e = table.get((min(u, v), max(u, v)))
                    if e is None:
                        n_missing += 1
                    else:
                        samples[e] += [float(data[z, y, x]), float(data[zz, yy, xx])]
    out = np.zeros((len(table), N_FEATS))
    for e, s in enumerate(samples):
        out[e] = row_of(s, len(s) // 2)
    return out, n_missing


def merge_features(n_edges, blocks):
    """`ndist.mergeFeatureBlocks` restated: blocks = [(edge_ids (m,), features (m, 10)), ...] ->
    (n_edges, 10).  count = sum w; mean and the quantiles are averages weighted with w = count;
    variance = sum w (var + (mean_r - mean)^2) / count; min / max over the rows with w > 0; an
    edge without any row stays 0."""
    ids = np.concatenate([np.asarray(i, dtype=np.int64) for i, _ in blocks] + [np.zeros(0, np.int64)])
    rows = np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1, N_FEATS) for _, f in blocks]
                          + [np.zeros((0, N_FEATS))])
    out = np.zeros((n_edges, N_FEATS))
    w = rows[:, 9]
    count = np.bincount(ids, weights=w, minlength=n_edges)
    has = count > 0
    div = np.where(has, count, 1.)
    for col in (0, 3, 4, 5, 6, 7):
        out[:, col] = np.bincount(ids, weights=w * rows[:, col], minlength=n_edges) / div
    out[:, 1] = np.bincount(ids, weights=w * (rows[:, 1] + (rows[:, 0] - out[ids, 0]) ** 2), minlength=n_edges) / div
    pos = w > 0
    lo, hi = np.full(n_edges, np.inf), np.full(n_edges, -np.inf)
    np.minimum.at(lo, ids[pos], rows[pos, 2])
    np.maximum.at(hi, ids[pos], rows[pos, 8])
    out[:, 2], out[:, 8] = np.where(has, lo, 0.), np.where(has, hi, 0.)
    out[:, 9] = count
    return out


def core_shape(blocking, block_id):
    block = blocking.getBlock(block_id)
    return tuple(int(e - b) for b, e in zip(block.begin, block.end))


def compare(got, ref):
    """count, min and max equal; mean, variance and the quantiles within 1e-10 absolute (the
    derivation is in test_edge_features_gpu.py)."""
    assert got.dtype == np.float64 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    for col in (9, 2, 8):
        np.testing.assert_array_equal(got[:, col], ref[:, col], err_msg='column %i' % col)
    for col in (0, 1, 3, 4, 5, 6, 7):
        np.testing.assert_allclose(got[:, col], ref[:, col], rtol=0, atol=1e-10, err_msg='column %i' % col)
