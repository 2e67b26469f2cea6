"""The numpy restatement of the reference's downscaling with `library: 'skimage'`
(cluster_tools/downscaling/downscaling.py:222-294): `skimage.measure.block_reduce` of the float32
block, then clip, round, cast -- and the block loop around it.  numpy only; it is the expected value
of the GPU and workflow tests, and tests/test_downscaling_ref.py holds it against recorded skimage
outputs (tests/golden/downscale_skimage.npz)."""
import numpy as np

from cluster_tools_amd.utils import volume_utils as vu
from cluster_tools_amd.utils.blocking import Blocking

FUNCS = ('mean', 'max', 'min')


def cells(x, factors):
    """x as float32, zero-padded at the end of every axis to a multiple of its factor and viewed
    as (oz, fz, oy, fy, ox, fx)."""
    x = np.asarray(x)
    assert x.ndim == 3 and len(factors) == 3
    x = x.astype(np.float32)  # (float64: round to nearest)
    pad = [(0, -n % f) for n, f in zip(x.shape, factors)]
    x = np.pad(x, pad, mode='constant', constant_values=0)
    oz, oy, ox = (n // f for n, f in zip(x.shape, factors))
    return x.reshape(oz, factors[0], oy, factors[1], ox, factors[2])


def reduce_block(x, factors, func='mean', dtype=None):
    """block_reduce(float32(x), factors, np.<func>) clipped, rounded and cast to `dtype` (x's own
    by default).  The mean is float32(S) / float32(n): S the cell's float64 sum, padded zeros
    included, rounded once to float32 (exact for the integer dtypes), n = fz fy fx."""
    assert func in FUNCS
    dtype = np.dtype(np.asarray(x).dtype if dtype is None else dtype)
    c = cells(x, factors)
    if func == 'mean':
        n = np.float32(int(np.prod(factors)))
        s = c.astype(np.float64).sum(axis=(1, 3, 5))
        out = s.astype(np.float32) / n
    else:
        out = getattr(c, func)(axis=(1, 3, 5))
    assert out.dtype == np.float32
    if dtype in (np.dtype('uint8'), np.dtype('uint16')):
        out = np.round(np.clip(out, 0, np.iinfo(dtype).max))
    return out.astype(dtype)


def downscale_volume(vol, out_shape, block_shape, scale_factor, halo=None, func='mean'):
    """The reference's `_ds_block` over every block of the output: `vol` (3-D, or 4-D with
    channels first) -> the level of shape `out_shape` (per channel).  scale_factor is an int or
    [fz, fy, fx]; halo is in input voxels, as the task takes it.  Blocks whose input box is all
    zero are skipped (they stay zero).  Also returns the ids of the skipped blocks."""
    vol = np.asarray(vol)
    factors = [scale_factor] * 3 if isinstance(scale_factor, int) else list(scale_factor)
    with_channels = vol.ndim == 4
    in_shape = vol.shape[1:] if with_channels else vol.shape
    lead = (slice(None),) if with_channels else ()
    out = np.zeros((vol.shape[:1] if with_channels else ()) + tuple(out_shape), dtype=vol.dtype)
    blocking = Blocking([0, 0, 0], list(out_shape), list(block_shape))
    skipped = []
    for block_id in range(blocking.numberOfBlocks):
        if halo is None:
            outer = inner = blocking.getBlock(block_id)
            local_bb = np.s_[:, :, :]
        else:
            b = blocking.getBlockWithHalo(block_id, [ha // sf for sf, ha in zip(factors, halo)])
            outer, inner, local_bb = b.outerBlock, b.innerBlock, vu.block_to_bb(b.innerBlockLocal)
        in_bb = tuple(slice(b * sf, min(e * sf, sh)) for b, e, sf, sh in zip(outer.begin, outer.end, factors, in_shape))
        x = vol[lead + in_bb]
        if np.sum(x != 0) == 0:
            skipped.append(block_id)
            continue
        red = np.stack([reduce_block(c, factors, func) for c in (x if with_channels else x[None])])
        assert red.shape[1:] == tuple(outer.shape), (red.shape, outer.shape)
        red = red[lead + local_bb] if with_channels else red[0][local_bb]
        out[lead + vu.block_to_bb(inner)] = red
    return out, skipped
