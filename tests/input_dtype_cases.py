"""Shared, GPU-free cases of the input dtype matrix: every raw dtype (uint8, uint16, float64; float32
as the control) on every normalize / x-pass kernel path of run_batch.

read_data_ref is the independent reference for `fin`: the reference's `_read_data` + `vu.normalize`
(+ the mask of `_ws_block`) in plain numpy.  as_dtype turns a float32 map in [0, 1] into one that
stresses the type.  The shapes are the smallest that reach each path; `prep_kernel` (the handle's
timings, include/ctws.h) names the x-pass kernel a test means to hit.

Typed batches take the foreground-bits kernel only when 2 * TF <= T (run_batch), T the voxels and
TF the frontier bitmap's words: max(ceil(Z Y / 64) * 64 * W, chunks * 64) with W = ceil(X / 64)
words per row and, in the 2-D watershed, chunks = W * ceil(Y / 64) * Z:
    (3, 20, 200): W 4,  TF = max(256, 12 * 64)  =  768, 2 TF =  1536 <= T = 12000
    (3, 12, 300): W 5,  TF = max(320, 15 * 64)  =  960, 2 TF =  1920 <= T = 10800
    (2, 10, 600): W 10, TF = max(640, 20 * 64)  = 1280, 2 TF =  2560 <= T = 12000
    (2, 8, 1100): rows > 1024, the generic kernel whatever TF is
(3-D watershed, D3 on (3, 20, 200): chunks = W * ceil(Y / 8) * ceil(Z / 8) = 12, the same 768.)
"""
import numpy as np

from cluster_tools_amd.synthetic import boundary_map, ellipsoid_mask

BLOCK_SHAPE = (64, 256, 256)
DTYPES = ('uint8', 'uint16', 'float64')

# the non-final y pass; the volumes are 2 to 3 slices deep, so z is not smoothed (sigma 2 needs 7 voxels)
D3 = dict(apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=(0., 2., 2.), sigma_weights=(0., 2., 2.))


def read_data_ref(x, config, mask=None):
    """The normalized input of `_ws_block` for the raw block x (3-D, or 4-D C, Z, Y, X)."""
    x = np.asarray(x)
    if x.ndim == 4:
        x = x[config.get('channel_begin', 0):config.get('channel_end', None)]
    v = x.astype('float32')
    v -= v.min()
    mx = v.max()
    if mx > 0:
        v /= mx
    if x.ndim == 4:
        v = getattr(np, config.get('agglomerate_channels', 'mean'))(v, axis=0)
    if config.get('invert_inputs', False):
        v = 1. - v
    if mask is not None:
        v[~np.asarray(mask).astype(bool)] = 1
    assert v.dtype == np.float32
    return v


def as_dtype(x, dtype):
    """A float32 map in [0, 1] as `dtype`, with values that stress the type: uint8 with a minimum
    above 0 and a maximum below 255; uint16 using both bytes up to 65535 (read as bytes or as uint8
    it differs everywhere); float64 values that float32 cannot represent, so that the order "cast,
    then normalize" matters."""
    dtype = np.dtype(dtype)
    x = np.asarray(x, dtype=np.float32)
    if dtype == np.uint8:
        return (3 + np.round(240 * x)).astype(np.uint8)
    if dtype == np.uint16:
        return (1000 + np.round(64535 * x)).astype(np.uint16)
    if dtype == np.float64:
        return 3.7 * x.astype(np.float64) - 1.1 + 1e-9
    assert dtype == np.float32
    return x


# 3-D shapes: name -> (shape, prep_kernel on the default handle, on a CTWS_EDT_BITS=0 handle)
SHAPES_3D = {
    'co4': ((3, 20, 200), 104, 4),      # 200 = 3 words + a tail of 8
    'co8': ((3, 12, 300), 108, 8),
    'co16': ((2, 10, 600), 116, 16),
    'generic': ((2, 8, 1100), 0, 0),    # rows > 1024
}
SHAPE_4D = (3, 20, 70)
CONFIGS_4D = {
    'mean': {},
    'max_begin1': dict(agglomerate_channels='max', channel_begin=1),
    'min_end3': dict(agglomerate_channels='min', channel_end=3),
    'range_invert': dict(channel_begin=1, channel_end=3, invert_inputs=True, threshold=.3),
    'neg_begin': dict(channel_begin=-3),
}
# the float32 control of k_prep_edt_x_reg<4> (CTWS_EDT_BITS=0 handle): prep_kernel 204
SHAPE_REG = (2, 8, 256)

_F32 = {}


def base_f32(shape, seed=None):
    """The float32 boundary map of a 3-D shape (computed once; do not modify)."""
    seed = sum(shape) if seed is None else seed
    key = (tuple(shape), seed)
    if key not in _F32:
        _F32[key] = boundary_map(tuple(shape), seed=seed)
        _F32[key].setflags(write=False)
    return _F32[key]


def base_4d():
    """4 channels of SHAPE_4D, seeds 4 to 7, float32."""
    return np.stack([base_f32(SHAPE_4D, seed=s) for s in (4, 5, 6, 7)])


def block_3d(name, dtype):
    return as_dtype(base_f32(SHAPES_3D[name][0]), dtype)


def block_4d(dtype):
    return as_dtype(base_4d(), dtype)


def stage_cases():
    """name -> (config, block dict, prep_kernel default handle, prep_kernel CTWS_EDT_BITS=0 handle):
    every dtype on the five paths, a mask per dtype on the co<8> shape and the 3-D config per
    dtype on the co<4> shape."""
    cases = {}
    for dt in DTYPES:
        for name, (shape, k_bits, k_old) in SHAPES_3D.items():
            cases['%s-%s' % (name, dt)] = ({}, dict(input=block_3d(name, dt)), k_bits, k_old)
        for name, cfg in CONFIGS_4D.items():
            cases['4d_%s-%s' % (name, dt)] = (cfg, dict(input=block_4d(dt)), 0, 0)
        shape, k_bits, k_old = SHAPES_3D['co8']
        cases['mask_co8-%s' % dt] = ({}, dict(input=block_3d('co8', dt), mask=ellipsoid_mask(shape)), k_bits, k_old)
        shape, k_bits, k_old = SHAPES_3D['co4']
        cases['d3_co4-%s' % dt] = (D3, dict(input=block_3d('co4', dt)), k_bits, k_old)
    cases['reg4-float32'] = ({}, dict(input=base_f32(SHAPE_REG)), 104, 204)
    return cases
