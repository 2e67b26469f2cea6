"""numpy restatement of the image filter (include/ctws.h, ctws_image_filter).

vigra is not installed, so `vigra.filters.gaussianSmoothing`, `gaussianGradientMagnitude` and
`laplacianOfGaussian` are restated from their definition: separable convolution with Gaussian
(derivative) taps, reflected borders, double accumulation over ascending source positions,
float32 between the axes, axes in the order z, y, x.  Parity with vigra itself is unpinned."""
import math

import numpy as np

FILTERS = ('gaussianSmoothing', 'gaussianGradientMagnitude', 'laplacianOfGaussian')
ORDER = {'gaussianSmoothing': 0, 'gaussianGradientMagnitude': 1, 'laplacianOfGaussian': 2}


def radius(sigma, order):
    return max(1, int((3.0 + 0.5 * order) * sigma + 0.5))


def taps(sigma, order):
    """The 2 r + 1 taps for the offsets -r .. r (numpy's exp; the library's come from libm)."""
    r = radius(sigma, order)
    x = np.arange(-r, r + 1, dtype=np.float64)
    e = np.exp(-x * x / (2.0 * sigma * sigma))
    if order == 0:
        k = e / (math.sqrt(2.0 * math.pi) * sigma)
        return k / k.sum()
    k = -x * e if order == 1 else (x * x / (sigma * sigma) - 1.0) * e
    k = k - k.sum() / len(k)
    moment = (k * (-x) ** order).sum() / math.factorial(order)
    return k / moment


def normalize(x):
    """vu.normalize (utils/volume_utils.py:113-120) in float32."""
    f = x.astype('float32')
    f -= f.min()
    m = f.max()
    if m > 0:
        f /= m
    return f


def convolve_axis(f, k, axis):
    """out[i] = float32(sum over p = i - r .. i + r ascending of k[i - p] * double(f[reflect(p)]))."""
    r = len(k) // 2
    L = f.shape[axis]
    if L < r + 1:
        raise ValueError("axis %i holds %i voxels, fewer than the radius %i + 1" % (axis, L, r))
    pad = [(0, 0)] * f.ndim
    pad[axis] = (r, r)
    g = np.pad(f.astype(np.float64), pad, mode='reflect')
    acc = np.zeros(f.shape, dtype=np.float64)
    sl = [slice(None)] * f.ndim
    for m in range(2 * r + 1):  # source position p = i - r + m, tap k[i - p] = k at offset r - m
        sl[axis] = slice(m, m + L)
        acc = acc + k[2 * r - m] * g[tuple(sl)]
    return acc.astype(np.float32)


def apply_filter(x, filter_name, sigma, apply_in_2d=False, do_normalize=True, taps_fn=taps):
    """The response of one block: float32, x's shape.  taps_fn(sigma, order) gives the taps (the GPU
    tests pass ctws.filter_taps, so that the convolution arithmetic compares bit for bit)."""
    order = ORDER[filter_name]
    if isinstance(sigma, (tuple, list)):
        assert len(sigma) == x.ndim and not apply_in_2d
        sig = [float(s) for s in sigma]
    else:
        sig = [float(sigma)] * x.ndim
    f = normalize(x) if do_normalize else x.astype('float32')
    if apply_in_2d:
        return np.stack([apply_filter(s, filter_name, sig[1], False, False, taps_fn) for s in f])
    axes = range(f.ndim)
    if order == 0:
        for a in axes:
            f = convolve_axis(f, taps_fn(sig[a], 0), a)
        return f
    comps = []
    for d in axes:  # the component with the derivative along d
        g = f
        for a in axes:
            g = convolve_axis(g, taps_fn(sig[a], order if a == d else 0), a)
        comps.append(g)
    if order == 1:
        s = comps[0] * comps[0]
        for g in comps[1:]:
            s = s + g * g
        return np.sqrt(s)  # float32, correctly rounded
    s = comps[0]
    for g in comps[1:]:
        s = s + g
    return s


def filter_blockwise(vol, block_shape, halo, filter_name, sigma, apply_in_2d=False, block_ids=None,
                     taps_fn=taps):
    """The reference's loop (features/image_filter.py:105-115): every block's outer box (the block
    grown by halo, clipped to the volume) normalized on its own and filtered, the inner box
    written.  Blocks not listed stay 0."""
    out = np.zeros(vol.shape, dtype=np.float32)
    grid = [(-(-s // b)) for s, b in zip(vol.shape, block_shape)]
    for bid in range(int(np.prod(grid))):
        if block_ids is not None and bid not in block_ids:
            continue
        pos = np.unravel_index(bid, grid)
        beg = [p * b for p, b in zip(pos, block_shape)]
        end = [min(b + bs, s) for b, bs, s in zip(beg, block_shape, vol.shape)]
        obeg = [max(b - h, 0) for b, h in zip(beg, halo)]
        oend = [min(e + h, s) for e, h, s in zip(end, halo, vol.shape)]
        outer = tuple(slice(b, e) for b, e in zip(obeg, oend))
        resp = apply_filter(vol[outer], filter_name, sigma, apply_in_2d, True, taps_fn)
        local = tuple(slice(b - ob, e - ob) for b, e, ob in zip(beg, end, obeg))
        out[tuple(slice(b, e) for b, e in zip(beg, end))] = resp[local]
    return out
