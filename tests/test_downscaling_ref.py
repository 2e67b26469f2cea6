"""The restatement of the downscaling (tests/downscaling_ref.py) against recorded
`skimage.measure.block_reduce` outputs (tests/golden/downscale_skimage.npz, written by
scripts/crosscheck_downscale_py39.py) and on crafted cells.  CPU only.

Integer dtypes, and max / min of every dtype, match skimage exactly.  Float means are held against
the exact mean M of the cell (fractions.Fraction), A the exact mean of |x|, zeros included:
* the restatement, which sums in float64: |got - M| <= 2^-23 (1 + 2^-20) |M| + n 2^-53 A -- the
  float64 sum ((n - 1) 2^-53 sum|x|), its rounding to float32 and the float32 division (2^-24
  each, relative, and their product);
* skimage, which sums in float32 in numpy's order: the same with the sum's unit roundoff 2^-24 in
  place of 2^-53, |got - M| <= 2^-23 (1 + 2^-20) |M| + n 2^-24 A.  This is the deviation of this
  project's float means from the reference's."""
import os
from fractions import Fraction

import numpy as np
import pytest

import downscaling_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'downscale_skimage.npz')


def exact_means(x, factors):
    """Per cell (M, A) as Fractions: the mean and the mean of |x| over the zero-padded cell."""
    c = R.cells(x, factors)
    oz, fz, oy, fy, ox, fx = c.shape
    n = fz * fy * fx
    flat = c.transpose(0, 2, 4, 1, 3, 5).reshape(-1, n)
    out = []
    for cell in flat:
        vals = [Fraction(float(v)) for v in cell]
        out.append((sum(vals) / n, sum(abs(v) for v in vals) / n))
    return out, n


def float_bound(m, a, n, sum_roundoff):
    return Fraction(2) ** -23 * (1 + Fraction(2) ** -20) * abs(m) + n * sum_roundoff * a


def worst_ratio(got, x, factors, sum_roundoff):
    """max over the cells of |got - M| / bound (0 / 0 counts as 0)."""
    means, n = exact_means(x, factors)
    worst = Fraction(0)
    for g, (m, a) in zip(np.asarray(got, dtype=np.float64).ravel(), means):
        err, bound = abs(Fraction(float(g)) - m), float_bound(m, a, n, sum_roundoff)
        assert err == 0 or bound > 0
        if err:
            worst = max(worst, err / bound)
    return float(worst)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_restatement_against_skimage(golden):
    cases = golden['cases']
    assert len(cases) == 32 and {c[0] for c in cases} == {'uint8', 'uint16', 'float32', 'float64'}
    for i, case in enumerate(cases):
        dtype, factors = case[0], tuple(int(f) for f in case[1:])
        x = golden['x%i' % i]
        assert str(x.dtype) == dtype
        for func in R.FUNCS:
            sk = golden['%s%i' % (func, i)]
            ref = R.reduce_block(x, factors, func, 'float32')
            assert ref.shape == sk.shape == tuple(-(-n // f) for n, f in zip(x.shape, factors))
            if dtype in ('uint8', 'uint16') or func != 'mean':
                np.testing.assert_array_equal(ref, sk, err_msg='%s %s %s' % (dtype, factors, func))
            else:
                assert worst_ratio(ref, x, factors, Fraction(2) ** -53) <= 1, (dtype, factors)
                assert worst_ratio(sk, x, factors, Fraction(2) ** -24) <= 1, (dtype, factors)
        if dtype in ('uint8', 'uint16'):
            # the cast result: skimage's float32 mean clipped, rounded and cast as `_ds_vol` does
            sk = golden['mean%i' % i]
            want = np.round(np.clip(sk, 0, np.iinfo(dtype).max)).astype(dtype)
            np.testing.assert_array_equal(R.reduce_block(x, factors, 'mean'), want)


@pytest.mark.parametrize('cell, want', [([0, 0, 1, 1], 0), ([1, 1, 2, 2], 2), ([2, 2, 3, 3], 2)])
def test_ties_round_half_to_even(cell, want):
    x = np.array(cell, dtype=np.uint8).reshape(1, 2, 2)
    assert R.reduce_block(x, (1, 2, 2), 'mean').tolist() == [[[want]]]


def test_padded_edge_cells():
    # the mean divides by n, not by the number of voxels inside the block
    x = np.full((1, 3, 3), 8, dtype=np.uint8)
    assert R.reduce_block(x, (1, 2, 2), 'mean').tolist() == [[[8, 4], [4, 2]]]
    # min is 0 at a padded edge of positive data
    assert R.reduce_block(x, (1, 2, 2), 'min').tolist() == [[[8, 0], [0, 0]]]
    assert R.reduce_block(x, (1, 2, 2), 'max').tolist() == [[[8, 8], [8, 8]]]
    # max is 0 at a padded edge of negative floats
    y = np.full((1, 3, 3), -2.5, dtype=np.float32)
    assert R.reduce_block(y, (1, 2, 2), 'max').tolist() == [[[-2.5, 0], [0, 0]]]
    assert R.reduce_block(y, (1, 2, 2), 'min').tolist() == [[[-2.5, -2.5], [-2.5, -2.5]]]
    assert R.reduce_block(y, (1, 2, 2), 'mean').tolist() == [[[-2.5, -1.25], [-1.25, -0.625]]]
    # a block smaller than one cell
    assert R.reduce_block(np.full((1, 1, 1), 200, dtype=np.uint8), (2, 2, 2), 'mean').tolist() == [[[25]]]


def test_float64_is_rounded_to_float32_first():
    x = np.full((1, 2, 2), 1 + 2. ** -30, dtype=np.float64)
    for func in R.FUNCS:
        out = R.reduce_block(x, (1, 2, 2), func)
        assert out.dtype == np.float64 and out.tolist() == [[[1.0]]]
    # float32 stays as it is
    z = np.full((1, 2, 2), np.float32(1 + 2. ** -23), dtype=np.float32)
    assert R.reduce_block(z, (1, 2, 2), 'mean')[0, 0, 0] == np.float32(1 + 2. ** -23)


@pytest.mark.parametrize('scale_factor, halo', [([1, 2, 2], None), ([1, 2, 2], [0, 4, 4]), (2, None), (2, [2, 2, 2])])
def test_downscale_volume_equals_one_reduction(scale_factor, halo):
    """With aligned blocks (the block's input box starts at a cell border) every output voxel sees
    the same cell whichever block computes it."""
    rng = np.random.RandomState(3)
    vol = rng.randint(1, 256, (20, 70, 66)).astype(np.uint8)  # (no zero block: nothing is skipped)
    factors = [scale_factor] * 3 if isinstance(scale_factor, int) else scale_factor
    whole = R.reduce_block(vol, factors, 'mean')
    got, skipped = R.downscale_volume(vol, whole.shape, [8, 32, 32], scale_factor, halo)
    assert skipped == []
    np.testing.assert_array_equal(got, whole)
    # an all-zero input box is skipped and stays zero
    vol[:16, :64, :64] = 0
    got, skipped = R.downscale_volume(vol, whole.shape, [8, 32, 32], scale_factor, None)
    assert 0 in skipped
    np.testing.assert_array_equal(got, R.reduce_block(vol, factors, 'mean'))
    # channels first
    vol4 = np.stack([vol, vol[::-1]])
    got4, _ = R.downscale_volume(vol4, whole.shape, [8, 32, 32], scale_factor, halo)
    np.testing.assert_array_equal(got4[1], R.reduce_block(vol[::-1], factors, 'mean'))
