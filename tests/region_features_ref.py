"""CPU restatement of RegionFeaturesWorkflow, in numpy and exact arithmetic,
for the tests: the block rows [id, count, mean] with exactly rounded sums (math.fsum), the
project's merge, the reference's float32 running-average merge restated, and the whole volume in
fractions.  Slow and plain on purpose."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53  # the unit roundoff of float64


def values(data):
    """The float32 value of every voxel: uint8 / 255, every other dtype cast (float64 rounds to
    nearest)."""
    data = np.asarray(data)
    if data.dtype == np.dtype('uint8'):
        return data.astype('float32') / np.float32(255.)
    return data.astype('float32')


def block_rows(labels, data, ignore_label=0):
    """rows (m, 3) float64 of [id, count, mean] for every id of the block, sorted by id; the sum is
    the exactly rounded float64 sum of the id's float32 values; the ignore label's row is
    [id, 0, 0]."""
    labels = np.asarray(labels)
    vals = values(data).astype('float64')
    assert labels.shape == vals.shape
    ids = np.unique(labels)
    rows = np.zeros((len(ids), 3), dtype='float64')
    for k, i in enumerate(ids):
        rows[k, 0] = float(i)
        if ignore_label is not None and int(i) == int(ignore_label):
            continue
        x = vals[labels == i]
        rows[k, 1] = float(len(x))
        rows[k, 2] = math.fsum(x.tolist()) / float(len(x))
    return rows


def merge(number_of_labels, tables):
    """The project's merge of the blocks' rows (in block order): per id count = sum n_b, mean =
    (sum of float64(n_b) * mean_b, in that order) / count, cast to float32; count 0 gives 0."""
    count = [0.0] * number_of_labels
    total = [0.0] * number_of_labels
    for t in tables:
        for i, n, mean in np.asarray(t).reshape(-1, 3):
            if not i < number_of_labels:
                raise RuntimeError("id %i, but number_of_labels is %i" % (int(i), number_of_labels))
            count[int(i)] += n
            total[int(i)] += n * mean
    out = np.zeros(number_of_labels, dtype='float64')
    for i in range(number_of_labels):
        if count[i] > 0:
            out[i] = total[i] / count[i]
    return out.astype('float32')


def merge_running_average(number_of_labels, tables):
    """The reference's merge (merge_region_features.py:92-127) restated: float32 chunks, and per
    block, for the ids of the block, the cumulative moving average in float32.  An id whose count
    stays 0 is left at 0 here (the reference divides 0 by 0 there)."""
    feats = np.zeros(number_of_labels, dtype='float32')
    counts = np.zeros(number_of_labels, dtype='float32')
    for t in tables:
        t = np.asarray(t).reshape(-1, 3).astype('float32')
        ids = t[:, 0].astype('uint64').astype('int64')
        n, mean = t[:, 1], t[:, 2]
        keep = n > 0
        ids, n, mean = ids[keep], n[keep], mean[keep]
        prev = counts[ids]
        tot = prev + n
        feats[ids] = (n * mean + prev * feats[ids]) / tot
        counts[ids] += n
    return feats


def volume_exact(labels, data, ignore_label=0):
    """{id: (n, sum of the float32 values as a Fraction, sum of their absolute values)} over the
    whole volume, the ignore label left out."""
    labels = np.asarray(labels)
    vals = values(data)
    out = {}
    for i in np.unique(labels):
        if ignore_label is not None and int(i) == int(ignore_label):
            continue
        x = vals[labels == i].astype('float64').tolist()
        out[int(i)] = (len(x), sum((Fraction(v) for v in x), Fraction(0)), sum((Fraction(abs(v)) for v in x), Fraction(0)))
    return out


def merged_mean_bound(max_block_count, k, n, abs_sum):
    """The bound on |mean - S / n| in float64 for an id held by k blocks, the largest of
    max_block_count voxels: (max n_b + k + 4) 2^-53 sum|x| / n -- the blocks' float64 sums in any
    order (n_b - 1 roundings each), their divisions, the k products, the k - 1 additions and the
    last division, with room for the second-order terms."""
    return Fraction(max_block_count + k + 4) * Fraction(U) * abs_sum / n
