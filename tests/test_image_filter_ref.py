"""The restatement of the image filter (tests/image_filter_ref.py) and the library's taps
(ctws.filter_taps, host code).  CPU only.

vigra is not installed, so the normalisation of the derivative kernels is pinned by polynomial
identities instead of anyone's memory of vigra: a Gaussian derivative filter of a polynomial of
degree <= 2 gives the polynomial's derivative exactly (away from the borders), whatever sigma.  The
bounds: float32 roundings of at most 2^-24 |v| (|v| <= 200 for the linear input, <= 1,200 for the
quadratic one) pass through taps whose absolute sum is about 1 over three axes: about 5e-5 and
5e-4; the bounds carry a 20x margin.  scipy is a second, deliberately loose cross-check: it neither
removes the DC part of a derivative kernel nor renormalises its moment."""
import math

import numpy as np
import pytest
from scipy import ndimage

from cluster_tools_amd import ctws
import image_filter_ref as R

SIGMAS = (0.5, 0.7, 1.0, 1.6, 2.5, 4.0)


@pytest.mark.parametrize('order', (0, 1, 2))
@pytest.mark.parametrize('sigma', SIGMAS)
def test_filter_taps(sigma, order):
    k = ctws.filter_taps(sigma, order)
    want = R.taps(sigma, order)
    r = R.radius(sigma, order) if order else max(1, int(3.0 * sigma + 0.5))
    assert k.dtype == np.float64 and len(k) == len(want) == 2 * r + 1
    assert np.abs(k - want).max() <= 1e-14 * np.abs(want).max()
    x = np.arange(-r, r + 1, dtype=np.float64)
    if order == 0:
        assert abs(k.sum() - 1.0) <= 1e-15 * (2 * r + 1)
    else:
        assert abs(k.sum()) <= 1e-15 * (2 * r + 1)
        moment = (k * (-x) ** order).sum() / math.factorial(order)
        assert abs(moment - 1.0) <= 1e-14
    if order == 1:  # (odd up to the removed mean, which is a rounding residue of an odd sum)
        assert np.abs(k + k[::-1]).max() <= 1e-15 * np.abs(k).max()
        assert k[0] > 0 > k[-1]  # k(x) ~ -x e(x): a true convolution differentiates a ramp to +1
    else:
        np.testing.assert_array_equal(k, k[::-1])


def test_filter_taps_refusals():
    for sigma, order in ((0.0, 0), (-1.0, 1), (float('nan'), 0), (1.0, 3), (1.0, -1)):
        with pytest.raises(ValueError):
            ctws.filter_taps(sigma, order)


def _interior(a, r):
    return a[r:-r, r:-r, r:-r]


def test_linear_polynomial():
    z, y, x = np.meshgrid(np.arange(24.), np.arange(24.), np.arange(40.), indexing='ij')
    f = (3 * x + 2 * y - z).astype('float32')
    g = R.apply_filter(f, 'gaussianGradientMagnitude', 1.0, do_normalize=False)
    lap = R.apply_filter(f, 'laplacianOfGaussian', 1.0, do_normalize=False)
    assert g.dtype == lap.dtype == np.float32
    r = R.radius(1.0, 2)
    assert np.abs(_interior(g, r) - math.sqrt(14.0)).max() <= 1e-3
    assert np.abs(_interior(lap, r)).max() <= 1e-3


def test_quadratic_polynomial():
    z, y, x = np.meshgrid(np.arange(20.), np.arange(20.), np.arange(24.), indexing='ij')
    f = ((x * x + 2 * y * y - z * z) / 2).astype('float32')
    lap = R.apply_filter(f, 'laplacianOfGaussian', 1.0, do_normalize=False)
    assert np.abs(_interior(lap, R.radius(1.0, 2)) - 2.0).max() <= 1e-2


def test_constant_input():
    f = np.full((12, 12, 12), 0.75, dtype='float32')
    # (a constant survives the reflection: every voxel counts, the borders too)
    np.testing.assert_allclose(R.apply_filter(f, 'gaussianSmoothing', 1.0, do_normalize=False), 0.75, atol=1e-6)
    np.testing.assert_allclose(R.apply_filter(f, 'gaussianGradientMagnitude', 1.0, do_normalize=False), 0, atol=1e-6)
    np.testing.assert_allclose(R.apply_filter(f, 'laplacianOfGaussian', 1.0, do_normalize=False), 0, atol=1e-6)


def _scipy(f, sigma, order_vec, order):
    # mode='mirror' is vigra's reflect (no repeated border voxel); truncate so that the radius is ours
    r = R.radius(sigma, order)
    return ndimage.gaussian_filter(f.astype(np.float64), sigma, order=order_vec, mode='mirror',
                                   truncate=(r + 0.01) / sigma)


@pytest.mark.parametrize('sigma', (1.0, 1.6, 2.5))
def test_against_scipy(sigma):
    """Smoothing on [0, 1] data within 1e-6; the derivative filters within 1 % of scipy's largest
    response.  scipy's truncated order-2 kernel keeps a DC part c (its taps sum to -2.6e-4 at sigma
    1.6), which answers the data's mean mu with c mu per axis whatever the structure.  In 1-D on
    [0, 1] noise that stays inside the bound (measured: at most 0.57 % over the three sigmas, at
    sigma 1.6, order 2).  In 3-D three axes add their DC parts while the noise's response shrinks
    (0.06 at sigma 1.6), and the artefact alone is 0.7 % of it -- 1.2 % was measured on [0, 1] noise
    -- so the 3-D comparison runs on the same noise centred at 0, where the artefact vanishes and
    the kernels' shapes are compared (measured: at most 0.60 %)."""
    rng = np.random.RandomState(3)
    f = rng.rand(20, 22, 24).astype('float32')
    got = R.apply_filter(f, 'gaussianSmoothing', sigma, do_normalize=False)
    assert np.abs(got - _scipy(f, sigma, 0, 0)).max() <= 1e-6
    f1 = rng.rand(400).astype('float32')
    want = np.abs(_scipy(f1, sigma, 1, 1))
    got = R.apply_filter(f1, 'gaussianGradientMagnitude', sigma, do_normalize=False)
    assert np.abs(got - want).max() <= 0.01 * want.max()
    want = _scipy(f1, sigma, 2, 2)
    got = R.apply_filter(f1, 'laplacianOfGaussian', sigma, do_normalize=False)
    assert np.abs(got - want).max() <= 0.01 * np.abs(want).max()
    # 3-D: each axis' kernel with our radius of that order; the other axes smooth with scipy's
    # order-0 kernel truncated at the derivative's radius (a tail below 1e-5 of the sum)
    f = f - np.float32(0.5)
    comps = [_scipy(f, sigma, tuple(1 if a == d else 0 for a in range(3)), 1) for d in range(3)]
    want = np.sqrt(sum(c * c for c in comps))
    got = R.apply_filter(f, 'gaussianGradientMagnitude', sigma, do_normalize=False)
    assert np.abs(got - want).max() <= 0.01 * np.abs(want).max()
    want = sum(_scipy(f, sigma, tuple(2 if a == d else 0 for a in range(3)), 2) for d in range(3))
    got = R.apply_filter(f, 'laplacianOfGaussian', sigma, do_normalize=False)
    assert np.abs(got - want).max() <= 0.01 * np.abs(want).max()


def test_normalize_restated():
    rng = np.random.RandomState(0)
    for dtype in ('uint8', 'uint16', 'float32', 'float64'):
        x = (rng.rand(5, 6, 7) * 200 + 3).astype(dtype)
        f = R.normalize(x)
        assert f.dtype == np.float32 and f.min() == 0.0 and f.max() == 1.0
        x32 = x.astype('float32')
        np.testing.assert_array_equal(f, (x32 - x32.min()) / np.float32(x32.max() - x32.min()))
    c = np.full((3, 4, 5), 7, dtype='uint8')
    np.testing.assert_array_equal(R.normalize(c), np.zeros((3, 4, 5), 'float32'))  # m = 0: no division
    neg = np.array([[[-2.0, 0.0, 6.0]]], dtype='float32')
    np.testing.assert_array_equal(R.normalize(neg), np.array([[[0.0, 0.25, 1.0]]], dtype='float32'))


@pytest.mark.parametrize('name', R.FILTERS)
def test_apply_in_2d_is_per_slice(name):
    rng = np.random.RandomState(1)
    x = rng.rand(3, 12, 14).astype('float32')
    got = R.apply_filter(x, name, 1.0, apply_in_2d=True)
    f = R.normalize(x)  # the block is normalized as a whole, then every slice is a 2-D image
    for z in range(3):
        want = R.apply_filter(f[z], name, 1.0, do_normalize=False)
        np.testing.assert_array_equal(got[z], want)
    assert got.shape == x.shape and got.dtype == np.float32


def test_sigma_list_and_short_axis():
    rng = np.random.RandomState(2)
    x = rng.rand(4, 12, 12).astype('float32')
    a = R.apply_filter(x, 'gaussianSmoothing', [0.5, 1.0, 1.0])
    f = R.normalize(x)
    for ax, s in enumerate((0.5, 1.0, 1.0)):
        f = R.convolve_axis(f, R.taps(s, 0), ax)
    np.testing.assert_array_equal(a, f)
    with pytest.raises(ValueError):
        R.apply_filter(x, 'gaussianSmoothing', 1.6)  # r = 5 along z of length 4
    with pytest.raises(AssertionError):
        R.apply_filter(x, 'gaussianSmoothing', [0.5, 1.0, 1.0], apply_in_2d=True)


def test_blockwise_equals_the_reference_loop():
    """filter_blockwise against the reference's loop written out with explicit boxes; per-block
    normalization makes it differ from the filter of the whole volume."""
    rng = np.random.RandomState(4)
    vol = (rng.rand(12, 16, 20) * 255).astype('uint8')
    bs, halo = (6, 8, 10), (2, 4, 4)
    got = R.filter_blockwise(vol, bs, halo, 'gaussianSmoothing', 1.0)
    want = np.zeros(vol.shape, 'float32')
    for z0 in range(0, 12, 6):
        for y0 in range(0, 16, 8):
            for x0 in range(0, 20, 10):
                oz, oy, ox = max(z0 - 2, 0), max(y0 - 4, 0), max(x0 - 4, 0)
                outer = vol[oz:min(z0 + 8, 12), oy:min(y0 + 12, 16), ox:min(x0 + 14, 20)]
                resp = R.apply_filter(outer, 'gaussianSmoothing', 1.0)
                want[z0:z0 + 6, y0:y0 + 8, x0:x0 + 10] = resp[z0 - oz:z0 - oz + 6, y0 - oy:y0 - oy + 8,
                                                             x0 - ox:x0 - ox + 10]
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(got, R.apply_filter(vol, 'gaussianSmoothing', 1.0))
    only = R.filter_blockwise(vol, bs, halo, 'gaussianSmoothing', 1.0, block_ids=[0, 7])
    np.testing.assert_array_equal(only[:6, :8, :10], want[:6, :8, :10])
    assert not only[:6, :8, 10:].any()
