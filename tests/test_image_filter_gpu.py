"""The image filter kernels (k_imgfilter.hip, ctws_image_filter) against the numpy restatement
(tests/image_filter_ref.py) fed with the library's own taps (ctws.filter_taps): the convolution,
normalization and combination arithmetic is compared bit for bit (assert_array_equal).

Shapes are the smallest at which each mechanism can fail: per axis r + 1 voxels (the smallest legal
line: every tap but the centre reflects), r + 2 and 17; rows of r + 1, 63, 64, 65 and 129 voxels (a
partial wave, a full one, a tail of 1, a second 64-lane group of the 256-wide row segment); lines
of 33 and 67 voxels (a second and third 32-row column tile); (5, 67, 1031) for several row segments
and x chunks.  sigma 4 with order 2 has radius 16, above the watershed's specialised range of 12:
one tile scheme with run-time radii serves every radius here, so there is no second path to name."""
import numpy as np
import pytest

from cluster_tools_amd import ctws
import image_filter_ref as R

pytestmark = pytest.mark.gpu

SIGMAS = [0.5, 1.0, 1.6, [0.5, 2.0, 2.0]]


def _ref(x, name, sigma, **kw):
    return R.apply_filter(x, name, sigma, taps_fn=ctws.filter_taps, **kw)


def _radii(name, sigma):
    sig = sigma if isinstance(sigma, list) else [sigma] * 3
    return [len(ctws.filter_taps(s, R.ORDER[name])) // 2 for s in sig]


def _check(h, x, name, sigma, **kw):
    got = h.image_filter(x, name, sigma, **kw)
    want = _ref(x, name, sigma, apply_in_2d=kw.get('apply_in_2d', False), do_normalize=kw.get('normalize', True))
    assert got.dtype == np.float32 and got.shape == x.shape
    np.testing.assert_array_equal(got, want, err_msg='%s sigma %s %s %s' % (name, sigma, x.shape, kw))
    return got


@pytest.mark.parametrize('sigma', SIGMAS, ids=str)
def test_shapes(gpu_handle, sigma):
    """Every row length under every filter, (nz, ny) rotating through r + 1, r + 2 and 17."""
    rng = np.random.RandomState(SIGMAS.index(sigma))
    k = SIGMAS.index(sigma)
    for name in R.FILTERS:
        rz, ry, rx = _radii(name, sigma)
        for nx in (rx + 1, 63, 64, 65, 129):
            nz = (rz + 1, rz + 2, 17)[k % 3]
            ny = (ry + 1, ry + 2, 17)[(k // 3) % 3]
            k += 1
            _check(gpu_handle, rng.rand(nz, ny, nx).astype('float32'), name, sigma)


def test_large_radius(gpu_handle):
    """sigma 4: radii 12 (order 0), 14 and 16 on the smallest block that holds them."""
    rng = np.random.RandomState(10)
    assert len(ctws.filter_taps(4.0, 2)) == 33
    for name in R.FILTERS:
        _check(gpu_handle, rng.rand(17, 17, 129).astype('float32'), name, 4.0)


@pytest.mark.parametrize('shape', [(5, 67, 1031), (33, 40, 65)], ids=str)
def test_more_than_one_tile(gpu_handle, shape):
    rng = np.random.RandomState(11)
    x = rng.rand(*shape).astype('float32')
    for name in R.FILTERS:
        _check(gpu_handle, x, name, 1.0)


@pytest.mark.parametrize('dtype', ('uint8', 'uint16', 'float32', 'float64'))
def test_input_dtypes_normalized(gpu_handle, dtype):
    rng = np.random.RandomState(12)
    shape = (9, 17, 65)
    if dtype in ('uint8', 'uint16'):
        x = rng.randint(3, np.iinfo(dtype).max - 5, shape).astype(dtype)
    else:
        x = (rng.rand(*shape) * 37.0 + 2.0).astype(dtype)
    for name in R.FILTERS:
        _check(gpu_handle, x, name, 1.0)
    const = np.full(shape, 7, dtype=dtype)  # m = 0: no division, a zero block
    for name in R.FILTERS:
        got = _check(gpu_handle, const, name, 1.0)
        assert not got.any()


def test_negative_values_and_no_normalize(gpu_handle):
    rng = np.random.RandomState(13)
    x = (rng.rand(9, 17, 65) * 10.0 - 6.0).astype('float32')
    for name in R.FILTERS:
        _check(gpu_handle, x, name, 1.0)
        got = _check(gpu_handle, x, name, 1.0, normalize=False)
        assert not np.array_equal(got, gpu_handle.image_filter(x, name, 1.0))


@pytest.mark.parametrize('nz', (1, 3))
def test_apply_in_2d(gpu_handle, nz):
    rng = np.random.RandomState(14)
    x = rng.rand(nz, 17, 65).astype('float32')  # z may be shorter than any radius: it is not filtered
    for name in R.FILTERS:
        _check(gpu_handle, x, name, 1.6, apply_in_2d=True)
    x = (rng.rand(nz, 40, 70) * 255).astype('uint8')
    _check(gpu_handle, x, 'gaussianGradientMagnitude', 1.0, apply_in_2d=True)


def test_short_axis_fails_and_leaves_the_handle_usable(gpu_handle):
    rng = np.random.RandomState(15)
    for axis, letter in enumerate('zyx'):
        shape = [9, 9, 9]
        shape[axis] = 4  # sigma 1, order 1: radius 4 needs 5 voxels
        with pytest.raises(ctws.CtwsError, match=r'axis %s holds 4 voxels, fewer than the radius 4 \+ 1' % letter):
            gpu_handle.image_filter(rng.rand(*shape).astype('float32'), 'gaussianGradientMagnitude', 1.0)
    with pytest.raises(ctws.CtwsError, match='radius of 51'):
        gpu_handle.image_filter(np.zeros((52, 52, 52), 'float32'), 'gaussianSmoothing', 17.0)
    _check(gpu_handle, rng.rand(5, 5, 5).astype('float32'), 'gaussianGradientMagnitude', 1.0)


def test_python_refusals(gpu_handle):
    x = np.zeros((8, 8, 8), 'float32')
    for name in ctws.MULTI_CHANNEL_FILTERS:
        with pytest.raises(NotImplementedError, match=name):
            gpu_handle.image_filter(x, name, 1.0)
    for args in (('gaussianBlur', 1.0), ('gaussianSmoothing', 0.0), ('gaussianSmoothing', [1.0, -1.0, 1.0]),
                 ('gaussianSmoothing', [1.0, 1.0])):
        with pytest.raises(ValueError):
            gpu_handle.image_filter(x, *args)
    with pytest.raises(ValueError, match='apply_in_2d'):
        gpu_handle.image_filter(x, 'gaussianSmoothing', [1.0, 1.0, 1.0], apply_in_2d=True)
    with pytest.raises(TypeError):
        gpu_handle.image_filter(x.astype('int32'), 'gaussianSmoothing', 1.0)


def test_device_tensors_and_repeats(gpu_handle):
    import torch
    rng = np.random.RandomState(16)
    for dtype in ('uint8', 'float32', 'float64'):
        x = (rng.rand(9, 33, 70) * 200).astype(dtype)
        for name in R.FILTERS:
            host = gpu_handle.image_filter(x, name, [0.5, 1.0, 1.6])
            t = torch.from_numpy(x).to('cuda:0')
            for _ in range(3):
                dev = gpu_handle.image_filter_device(t, name, [0.5, 1.0, 1.6])
                assert dev.is_cuda and dev.dtype == torch.float32
                np.testing.assert_array_equal(dev.cpu().numpy(), host)
            np.testing.assert_array_equal(gpu_handle.image_filter(x, name, [0.5, 1.0, 1.6]), host)
            np.testing.assert_array_equal(t.cpu().numpy(), x)  # the input is not written
    assert set(gpu_handle.timings()) == {'if_minmax', 'if_first', 'if_y', 'if_x'}
