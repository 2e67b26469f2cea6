"""The downscaling kernels (k_downscale.hip, ctws_downscale_block) against the numpy restatement
(tests/downscaling_ref.py) on the smallest shapes at which each mechanism can fail: rows of 1, 15,
16, 17, 63, 64, 65, 67 and 129 voxels (no vector group, one, a tail of 1, rows whose pitch is no
multiple of 16 bytes, a tail behind several groups) of 1, 2, 3 and 5 rows and slices (odd extents:
padded cells), the pyramid's own factors (the vector kernels) and six others (the cell kernel), four
dtypes, three functions.  Everything but the general float means is compared with
assert_array_equal: integers sum exactly, and the float inputs of the sweep are quarters whose sums
are exact in float64 and float32, so the one float32 division gives the restatement's bits.

General floats (both signs, magnitudes 2^-40 .. 2^40, no subnormals): per cell
|got - M| <= 2^-23 (1 + 2^-20) |M| + n 2^-53 A, M the exact mean, A the exact mean of |x|, zeros
included (fractions.Fraction) -- the float64 sum in a fixed order ((n - 1) 2^-53 sum|x|), its one
rounding to float32 and the one float32 division (2^-24 each, relative).  The largest ratio seen is
printed (profiles/downscaling/general_floats_error.txt keeps a copy)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from cluster_tools_amd import ctws
from cluster_tools_amd.ctws import lib
import downscaling_ref as R

pytestmark = pytest.mark.gpu

NX = (1, 15, 16, 17, 63, 64, 65, 67, 129)
NZY = [(nz, ny) for nz in (1, 2, 3, 5) for ny in (1, 2, 3, 5)]
FACTORS = [(1, 1, 1), (1, 2, 2), (2, 2, 2), (1, 3, 3), (3, 3, 3), (1, 4, 4), (4, 4, 4), (2, 3, 5)]
DTYPES = ('uint8', 'uint16', 'float32', 'float64')
UNSUPPORTED, EINVAL = -5, -1


def _values(rng, dtype, shape):
    if dtype in ('uint8', 'uint16'):
        return rng.randint(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
    return (rng.randint(-1024, 1025, shape) / 4.).astype(dtype)  # quarters: every sum is exact


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('factors', FACTORS, ids=lambda f: '%ix%ix%i' % f)
def test_shapes(gpu_handle, factors, dtype):
    """Every row length, with (nz, ny) rotating through all sixteen pairs, every function."""
    rng = np.random.RandomState(FACTORS.index(factors) * 4 + DTYPES.index(dtype))
    k = 5 * FACTORS.index(factors) + DTYPES.index(dtype)
    for func in R.FUNCS:
        for nx in NX:
            nz, ny = NZY[k % 16]
            k += 1
            x = _values(rng, dtype, (nz, ny, nx))
            got, nonzero = gpu_handle.downscale_block(x, factors, func)
            want = R.reduce_block(x, factors, func)
            assert got.dtype == x.dtype and got.shape == want.shape
            np.testing.assert_array_equal(got, want, err_msg='%s %s %s' % (func, factors, x.shape))
            assert nonzero == bool((x != 0).any())


@pytest.mark.parametrize('factors', [(1, 2, 2), (2, 2, 2), (3, 3, 3)], ids=lambda f: '%ix%ix%i' % f)
def test_more_than_one_workgroup(gpu_handle, factors):
    """(5, 67, 1031): several workgroups, groups and a tail in every row, padded cells on all axes."""
    rng = np.random.RandomState(1)
    for dtype in DTYPES:
        x = _values(rng, dtype, (5, 67, 1031))
        for func in ('mean', 'min'):
            got, nonzero = gpu_handle.downscale_block(x, factors, func)
            np.testing.assert_array_equal(got, R.reduce_block(x, factors, func))
            assert nonzero


def test_uint16_exactness_limit(gpu_handle):
    """(8, 8, 4) on all-65535 uint16: the cell's sum is 2^24 - 256, the last exact one."""
    x = np.full((9, 17, 9), 65535, dtype=np.uint16)
    got, _ = gpu_handle.downscale_block(x, (8, 8, 4), 'mean')
    want = R.reduce_block(x, (8, 8, 4), 'mean')
    assert want[0, 0, 0] == 65535 and want[1, 2, 2] == round(65535 / 256)
    np.testing.assert_array_equal(got, want)
    # (8, 8, 8): n max = 2^25 - 512, refused with nothing written; max and min are exact there
    out = np.full((2, 3, 2), 7, dtype=np.uint16)
    ret, flag = gpu_handle.downscale_block_raw(x, (8, 8, 8), 0, out)
    assert ret == UNSUPPORTED and flag == 0 and (out == 7).all()
    assert '2^24' in gpu_handle.last_error()
    with pytest.raises(ctws.CtwsError, match='2\\^24'):
        gpu_handle.downscale_block(x, (8, 8, 8), 'mean')
    for func in ('max', 'min'):
        got, _ = gpu_handle.downscale_block(x, (8, 8, 8), func)
        np.testing.assert_array_equal(got, R.reduce_block(x, (8, 8, 8), func))
    y = np.full((9, 17, 9), 255, dtype=np.uint8)
    np.testing.assert_array_equal(gpu_handle.downscale_block(y, (8, 8, 8), 'mean')[0], R.reduce_block(y, (8, 8, 8)))


@pytest.mark.parametrize('dtype', DTYPES)
def test_value_cases(gpu_handle, dtype):
    """The crafted cells of tests/test_downscaling_ref.py, for every dtype and function."""
    h = gpu_handle
    for cell, want in (([0, 0, 1, 1], 0), ([1, 1, 2, 2], 2), ([2, 2, 3, 3], 2)):
        x = np.array(cell, dtype=dtype).reshape(1, 2, 2)
        got = h.downscale_block(x, (1, 2, 2), 'mean')[0]
        # ties round half to even for the integers; floats keep the half
        assert got.tolist() == [[[want if dtype.startswith('uint') else sum(cell) / 4.]]]
        assert h.downscale_block(x, (1, 2, 2), 'max')[0].tolist() == [[[max(cell)]]]
        assert h.downscale_block(x, (1, 2, 2), 'min')[0].tolist() == [[[min(cell)]]]
    x = np.full((1, 3, 3), 8, dtype=dtype)
    assert h.downscale_block(x, (1, 2, 2), 'mean')[0].tolist() == [[[8, 4], [4, 2]]]  # divides by n
    assert h.downscale_block(x, (1, 2, 2), 'min')[0].tolist() == [[[8, 0], [0, 0]]]
    assert h.downscale_block(x, (1, 2, 2), 'max')[0].tolist() == [[[8, 8], [8, 8]]]
    # a block smaller than one cell
    one = np.full((1, 1, 1), 200, dtype=dtype)
    assert h.downscale_block(one, (2, 2, 2), 'mean')[0].tolist() == [[[25]]]
    assert h.downscale_block(one, (2, 2, 2), 'max')[0].tolist() == [[[200]]]
    assert h.downscale_block(one, (2, 2, 2), 'min')[0].tolist() == [[[0]]]
    if dtype.startswith('float'):
        y = np.full((1, 3, 3), -2.5, dtype=dtype)
        assert h.downscale_block(y, (1, 2, 2), 'max')[0].tolist() == [[[-2.5, 0], [0, 0]]]
        assert h.downscale_block(y, (1, 2, 2), 'min')[0].tolist() == [[[-2.5] * 2] * 2]
        assert h.downscale_block(y, (1, 2, 2), 'mean')[0].tolist() == [[[-2.5, -1.25], [-1.25, -0.625]]]
    if dtype == 'float64':
        z = np.full((1, 2, 2), 1 + 2. ** -30, dtype=np.float64)  # rounded to float32 first
        for func in R.FUNCS:
            for factors in ((1, 2, 2), (1, 1, 1)):
                got = h.downscale_block(z, factors, func)[0]
                assert got.dtype == np.float64 and (got == 1.0).all()


def _wide_floats(rng, shape):
    """float32 of both signs with magnitudes in [2^-40, 2^40): no subnormals, no exact sums."""
    mant = 1 + rng.randint(0, 2 ** 23, shape) * 2. ** -23
    sign = np.where(rng.rand(*shape) < .5, -1., 1.)
    return (sign * mant * np.exp2(rng.randint(-40, 40, shape))).astype(np.float32)


def test_general_floats(gpu_handle):
    rng = np.random.RandomState(5)
    worst = Fraction(0)
    for factors, shape in (((1, 2, 2), (3, 5, 67)), ((2, 2, 2), (5, 7, 65)), ((3, 3, 3), (5, 8, 31)),
                           ((2, 3, 5), (5, 7, 33)), ((8, 8, 8), (9, 17, 19)), ((4, 4, 4), (5, 9, 34))):
        x = _wide_floats(rng, shape)
        n = int(np.prod(factors))
        c = R.cells(x, factors).transpose(0, 2, 4, 1, 3, 5).reshape(-1, n)
        for dtype in ('float32', 'float64'):
            got, _ = gpu_handle.downscale_block(x.astype(dtype), factors, 'mean')
            assert got.dtype == np.dtype(dtype) and got.size == len(c)
            for g, cell in zip(got.ravel(), c):
                vals = [Fraction(float(v)) for v in cell]
                m, a = sum(vals) / n, sum(abs(v) for v in vals) / n
                bound = Fraction(2) ** -23 * (1 + Fraction(2) ** -20) * abs(m) + n * Fraction(2) ** -53 * a
                err = abs(Fraction(float(g)) - m)
                assert err <= bound, (factors, dtype, float(g), float(m), float(err / bound))
                if bound:
                    worst = max(worst, err / bound)
    print("general floats: largest |got - M| / bound = %.4f" % float(worst))
    assert 0 < worst <= 1


def test_any_nonzero(gpu_handle):
    for dtype in DTYPES:
        for factors in ((2, 2, 2), (1, 2, 2), (3, 3, 3)):
            x = np.zeros((5, 7, 67), dtype=dtype)
            got, nonzero = gpu_handle.downscale_block(x, factors)
            assert nonzero is False and not got.any()
            x[-1, -1, -1] = 1  # one nonzero voxel at the last position (a padded cell)
            got, nonzero = gpu_handle.downscale_block(x, factors)
            assert nonzero is True
            np.testing.assert_array_equal(got, R.reduce_block(x, factors))
            x[-1, -1, -1] = 0
            x[2, 3, 40] = 3  # and inside a vector group
            assert gpu_handle.downscale_block(x, factors)[1] is True
    for dtype in ('float32', 'float64'):
        x = np.full((3, 4, 70), -0.0, dtype=dtype)  # -0.0 is zero
        assert np.signbit(x).all()
        for factors in ((2, 2, 2), (3, 3, 3)):
            got, nonzero = gpu_handle.downscale_block(x, factors)
            assert nonzero is False and not got.any()


def test_repeatability_and_device_form(gpu_handle):
    import torch
    rng = np.random.RandomState(9)
    for factors, shape in (((2, 2, 2), (5, 9, 131)), ((1, 2, 2), (3, 9, 64)), ((2, 3, 5), (5, 9, 131))):
        for dtype in DTYPES:
            x = _wide_floats(rng, shape).astype(dtype) if dtype.startswith('float') else _values(rng, dtype, shape)
            first, flag = gpu_handle.downscale_block(x, factors)
            for _ in range(4):
                again, flag2 = gpu_handle.downscale_block(x, factors)
                assert again.tobytes() == first.tobytes() and flag2 == flag
            t = torch.from_numpy(x.view(np.int16) if dtype == 'uint16' else x).to('cuda:0')
            if dtype == 'uint16':
                t = t.view(torch.uint16)
            out, flag3 = gpu_handle.downscale_block_device(t, factors)
            assert out.is_cuda and out.dtype == t.dtype and tuple(out.shape) == first.shape and flag3 == flag
            host = out.view(torch.int16).cpu().numpy().view(np.uint16) if dtype == 'uint16' else out.cpu().numpy()
            assert host.tobytes() == first.tobytes()


def test_python_refusals(gpu_handle):
    h = gpu_handle
    x = np.ones((2, 4, 4), dtype=np.uint8)
    for dtype in ('uint32', 'uint64', 'int8', 'float16', 'bool'):
        with pytest.raises(TypeError, match='uint8, uint16, float32 or float64, not %s' % dtype):
            h.downscale_block(x.astype(dtype), (1, 2, 2))
    for bad in (np.ones((4, 4), 'uint8'), np.ones((1, 2, 4, 4), 'uint8'), np.ones((2, 0, 4), 'uint8')):
        with pytest.raises(ValueError, match='non-empty 3-D block'):
            h.downscale_block(bad, (1, 2, 2))
    for factors in ((2, 2), (1, 2, 2, 2), (0, 2, 2), (1, 2, 9), (1, 2.5, 2), 2, (1, -2, 2)):
        with pytest.raises(ValueError, match='three integers in 1..8'):
            h.downscale_block(x, factors)
    with pytest.raises(ValueError, match="'mean', 'max' or 'min', not 'median'"):
        h.downscale_block(x, (1, 2, 2), 'median')
    # the library's own checks: wrong output extents, a factor out of range, an unknown function
    out = np.full((2, 2, 3), 9, dtype=np.uint8)
    assert h.downscale_block_raw(x, (1, 2, 2), 0, out)[0] == EINVAL and 'ceil(n / f)' in h.last_error()
    out = np.full((2, 2, 2), 9, dtype=np.uint8)
    assert h.downscale_block_raw(x, (1, 2, 9), 0, np.full((2, 2, 1), 9, np.uint8))[0] == EINVAL
    assert h.downscale_block_raw(x, (1, 2, 2), 3, out)[0] == EINVAL
    assert (out == 9).all()
    assert h.downscale_block_raw(x, (1, 2, 2), 0, out) == (0, 1) and (out == 1).all()


def test_block_limit(gpu_handle):
    """2^31 voxels or more are refused through the raw entry point before any memory is touched:
    the buffers behind the pointers hold four voxels."""
    x = np.ones((1, 1, 4), dtype=np.float32)
    out = np.full((1, 1, 4), np.nan, dtype=np.float32)
    flag = C.c_int(-1)
    for shape in ((2 ** 31, 1, 1), (1, 2 ** 31, 1), (2 ** 16, 2 ** 15, 1), (2 ** 11, 2 ** 10, 2 ** 10)):
        for factors in ((1, 1, 1), (2, 2, 2)):
            oshape = [-(-n // f) for n, f in zip(shape, factors)]
            ret = lib().ctws_downscale_block(gpu_handle._h, x.ctypes.data, 3, *shape, (C.c_int64 * 3)(*factors), 0,
                                             out.ctypes.data, *oshape, C.byref(flag))
            assert ret == UNSUPPORTED and flag.value == 0 and np.isnan(out).all(), shape
            assert '2^31' in gpu_handle.last_error()
