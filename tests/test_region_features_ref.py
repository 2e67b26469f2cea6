"""CPU tests of the RegionFeaturesWorkflow restatement (tests/region_features_ref.py): the block rows
against a triple loop, the merged blocks against the whole volume in exact arithmetic, and the
project's merge against the reference's float32 running average."""
from fractions import Fraction

import numpy as np
import pytest

from cluster_tools_amd.utils import volume_utils as vu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.features.merge_region_features import merge_rows
import region_features_ref as R

DTYPES = ['uint8', 'uint16', 'float32', 'float64']


def _data(rng, shape, dtype):
    if dtype == 'uint8':
        return rng.randint(0, 256, shape).astype('uint8')
    if dtype == 'uint16':
        return rng.randint(0, 65536, shape).astype('uint16')
    return rng.rand(*shape).astype(dtype)


def _loop_rows(labels, data, ignore_label):
    """The rows by a triple loop over the voxels, sums in fractions."""
    acc = {}
    for z in range(labels.shape[0]):
        for y in range(labels.shape[1]):
            for x in range(labels.shape[2]):
                i = int(labels[z, y, x])
                v = data[z, y, x]
                f = np.float32(v) / np.float32(255.) if data.dtype == np.dtype('uint8') else np.float32(v)
                n, s = acc.get(i, (0, Fraction(0)))
                acc[i] = (n + 1, s + Fraction(float(f)))
    rows = []
    for i in sorted(acc):
        n, s = acc[i]
        if ignore_label is not None and i == ignore_label:
            rows.append([float(i), 0., 0.])
        else:
            rows.append([float(i), float(n), float(s) / float(n)])  # (float(Fraction) rounds to nearest)
    return np.array(rows, dtype='float64')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('ignore_label', [0, 7, None])
def test_block_rows_equal_a_triple_loop(dtype, ignore_label):
    rng = np.random.RandomState(3)
    labels = rng.randint(0, 10, (3, 4, 5)).astype('uint64')
    data = _data(rng, labels.shape, dtype)
    got = R.block_rows(labels, data, ignore_label)
    np.testing.assert_array_equal(got, _loop_rows(labels, data, ignore_label))
    assert got.dtype == np.float64 and got.shape[1] == 3
    if ignore_label is not None:
        assert not got[got[:, 0] == ignore_label, 1:].any()


def test_values():
    assert R.values(np.array([255, 51], 'uint8')).tolist() == [1.0, float(np.float32(51) / np.float32(255))]
    assert R.values(np.array([65535], 'uint16')).tolist() == [65535.0]  # not scaled
    v = R.values(np.array([0.1, 1 + 2.0 ** -30], 'float64'))
    assert v.dtype == np.float32 and v.tolist() == [float(np.float32(0.1)), 1.0]


SHAPE, BLOCK_SHAPE = (10, 12, 20), [4, 8, 8]


def _blocks(signed):
    """Labels, data (signed: N(0, 9); else uniform in [0, 1), as the reference's test data), the
    blocks' tables, the number of blocks that hold each id and its largest count in one block."""
    rng = np.random.RandomState(5)
    coarse = rng.randint(0, 9, (5, 4, 5)).astype('uint64')
    labels = np.kron(coarse, np.ones((2, 3, 4), dtype='uint64'))
    assert labels.shape == SHAPE
    data = ((rng.randn(*SHAPE) * 3) if signed else rng.rand(*SHAPE)).astype('float32')
    blocking = Blocking([0, 0, 0], list(SHAPE), BLOCK_SHAPE)
    tables, holders, largest = [], {}, {}
    for block_id in range(blocking.numberOfBlocks):
        bb = vu.block_to_bb(blocking.getBlock(block_id))
        t = R.block_rows(labels[bb], data[bb], 0)
        tables.append(t)
        for i, n, _ in t:
            holders[int(i)] = holders.get(int(i), 0) + 1
            largest[int(i)] = max(largest.get(int(i), 0), int(n))
    return labels, data, tables, holders, largest


def test_merged_blocks_equal_the_whole_volume():
    labels, data, tables, holders, largest = _blocks(True)
    exact = R.volume_exact(labels, data, 0)
    n_labels = 12
    rows = np.concatenate(tables)
    got64 = np.zeros(n_labels)
    # the float64 merge before its cast, as merge_rows takes it
    idx = rows[:, 0].astype('int64')
    count = np.bincount(idx, weights=rows[:, 1], minlength=n_labels)
    total = np.bincount(idx, weights=rows[:, 1] * rows[:, 2], minlength=n_labels)
    got64[count > 0] = total[count > 0] / count[count > 0]
    assert max(holders.values()) >= 4
    for i, (n, s, a) in exact.items():
        assert count[i] == n
        err = abs(Fraction(float(got64[i])) - s / n)
        assert err <= R.merged_mean_bound(largest[i], holders[i], n, a), (i, float(err))
    merged = merge_rows(rows, 0, n_labels)
    np.testing.assert_array_equal(merged, got64.astype('float32'))
    np.testing.assert_array_equal(merged, R.merge(n_labels, tables))
    assert merged.dtype == np.float32 and merged[0] == 0 and not merged[9:].any()


def test_our_merge_and_the_running_average_agree():
    _, _, tables, _, _ = _blocks(False)
    ours = R.merge(12, tables)
    theirs = R.merge_running_average(12, tables)
    assert np.allclose(ours, theirs)
    assert ours.any()
    # split into label ranges, as the jobs do
    rows = np.concatenate(tables)
    np.testing.assert_array_equal(np.concatenate([merge_rows(rows, 0, 5), merge_rows(rows, 5, 12)]), ours)
