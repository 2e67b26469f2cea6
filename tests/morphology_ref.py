"""CPU restatement of the morphology tables (nifty's
`computeAndSerializeMorphology` / `mergeAndSerializeMorphology` are not available):

    row = [id, n, com_z, com_y, com_x, min_z, min_y, min_x, max_z, max_y, max_x]

per id of a block (0 included) at the global coordinates begin + local, minima and maxima
inclusive, com = float(S) / float(n) with the coordinate sums S taken in integers."""
from fractions import Fraction

import numpy as np


def _axis_coords(shape, a):
    """The coordinate along axis a of every voxel, flat in C order, int64."""
    view = [1, 1, 1]
    view[a] = shape[a]
    return np.broadcast_to(np.arange(shape[a], dtype=np.int64).reshape(view), shape).ravel()


def block_morphology(labels, begin=(0, 0, 0)):
    """The (m, 11) float64 table of one block, sorted by id; vectorised, int64 sums."""
    labels = np.asarray(labels, dtype=np.uint64)
    assert labels.ndim == 3 and labels.size
    ids, inv = np.unique(labels.ravel(), return_inverse=True)
    inv = inv.ravel()
    m = len(ids)
    n = np.bincount(inv, minlength=m).astype(np.int64)
    out = np.zeros((m, 11), dtype=np.float64)
    out[:, 0] = ids.astype(np.float64)
    out[:, 1] = n.astype(np.float64)
    # the voxels grouped by id: each id's coordinates are one segment of the sorted order
    order = np.argsort(inv, kind='stable')
    starts = np.cumsum(n) - n
    for a in range(3):
        g = (_axis_coords(labels.shape, a) + int(begin[a]))[order]
        s = np.add.reduceat(g, starts)
        lo = np.minimum.reduceat(g, starts)
        hi = np.maximum.reduceat(g, starts)
        out[:, 2 + a] = np.array([float(int(si)) / float(int(ni)) for si, ni in zip(s, n)])
        out[:, 5 + a] = lo.astype(np.float64)
        out[:, 8 + a] = hi.astype(np.float64)
    return out


def block_morphology_brute(labels, begin=(0, 0, 0)):
    """The same table by a triple loop over the voxels (arrays up to 5 x 6 x 7)."""
    labels = np.asarray(labels, dtype=np.uint64)
    assert labels.ndim == 3 and labels.size <= 5 * 6 * 7
    acc = {}
    for z in range(labels.shape[0]):
        for y in range(labels.shape[1]):
            for x in range(labels.shape[2]):
                g = (z + int(begin[0]), y + int(begin[1]), x + int(begin[2]))
                e = acc.setdefault(int(labels[z, y, x]), [0, [0, 0, 0], list(g), list(g)])
                e[0] += 1
                for a in range(3):
                    e[1][a] += g[a]
                    e[2][a] = min(e[2][a], g[a])
                    e[3][a] = max(e[3][a], g[a])
    rows = [[float(i), float(n)] + [float(s) / float(n) for s in S] + [float(v) for v in lo] + [float(v) for v in hi]
            for i, (n, S, lo, hi) in sorted(acc.items())]
    return np.array(rows, dtype=np.float64).reshape(-1, 11)


def merge_morphology(number_of_labels, blocks):
    """The merged (number_of_labels, 11) table of the blocks' tables, taken in their order: size =
    the sum of the sizes, com = (the sum of float(size_b) * com_b in that order) / size, min / max
    over the rows; an id without a row keeps eleven zeros, an id out of range is an error."""
    out = np.zeros((number_of_labels, 11), dtype=np.float64)
    seen = np.zeros(number_of_labels, dtype=bool)
    for k, rows in enumerate(blocks):
        for row in np.asarray(rows, dtype=np.float64).reshape(-1, 11):
            i = int(row[0])
            if i >= number_of_labels:
                raise RuntimeError("id %i in block table %i, but number_of_labels is %i" % (i, k, number_of_labels))
            if not seen[i]:
                seen[i] = True
                out[i, 0] = row[0]
                out[i, 1] = row[1]
                out[i, 2:5] = row[1] * row[2:5]
                out[i, 5:] = row[5:]
            else:
                out[i, 1] += row[1]
                out[i, 2:5] += row[1] * row[2:5]
                out[i, 5:8] = np.minimum(out[i, 5:8], row[5:8])
                out[i, 8:] = np.maximum(out[i, 8:], row[8:])
    out[seen, 2:5] /= out[seen, 1:2]
    return out


def volume_exact(labels):
    """{id: (n, (S_z / n, S_y / n, S_x / n) as Fractions, (min_z, min_y, min_x), (max_z, max_y,
    max_x))} of a whole volume, in integers."""
    labels = np.asarray(labels, dtype=np.uint64)
    ids, inv = np.unique(labels.ravel(), return_inverse=True)
    inv = inv.ravel()
    n = np.bincount(inv, minlength=len(ids))
    order = np.argsort(inv, kind='stable')
    starts = np.cumsum(n) - n
    S, lo, hi = [], [], []
    for a in range(3):
        g = _axis_coords(labels.shape, a)[order]
        S.append(np.add.reduceat(g, starts))
        lo.append(np.minimum.reduceat(g, starts))
        hi.append(np.maximum.reduceat(g, starts))
    return {int(i): (int(n[k]), tuple(Fraction(int(S[a][k]), int(n[k])) for a in range(3)),
                     tuple(int(lo[a][k]) for a in range(3)), tuple(int(hi[a][k]) for a in range(3)))
            for k, i in enumerate(ids)}


def centre_bound(k, shape):
    """|merged centre - S / n| <= (k + 3) 2^-53 max(shape) for an id held by k blocks: the roundings
    of com_b, of the k products, of the k - 1 additions and of one division, each relative 2^-53 on
    a value of at most max(shape)."""
    return (k + 3) * 2.0 ** -53 * max(shape)
