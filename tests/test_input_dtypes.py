"""CPU: the oracle's `input` stage equals a numpy restatement of the reference's `_read_data` +
`vu.normalize` (tests/input_dtype_cases.py read_data_ref) bit for bit for every dtype, 3-D and 4-D
with channel ranges, masks included: the checker of the GPU's `fin` is pinned to the reference's
arithmetic independently of the GPU.  And `make_cfg` refuses a negative `channel_end`, which the
struct cannot tell from None."""
import numpy as np
import pytest

from cluster_tools_amd import _abi
from oracle import oracle as O
import input_dtype_cases as IC

CASES = IC.stage_cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_oracle_input_stage_equals_read_data_ref(name):
    config, block, _, _ = CASES[name]
    ref = O.ws_blocks(config, IC.BLOCK_SHAPE, [dict(block, block_id=3)], with_stages=True)[0]
    want = IC.read_data_ref(block['input'], config, block.get('mask'))
    assert ref['status'] == 0
    assert ref['input'].dtype == want.dtype == np.float32
    np.testing.assert_array_equal(ref['input'], want)
    # not degenerate: some foreground, not only foreground
    fg = (want > config.get('threshold', .5)).mean()
    assert 0 < fg < 1, fg


def test_as_dtype_stresses_the_type():
    x = IC.base_f32(IC.SHAPES_3D['co4'][0])
    u8, u16, f64 = (IC.as_dtype(x, d) for d in IC.DTYPES)
    assert u8.dtype == np.uint8 and 0 < u8.min() and u8.max() < 255
    assert u16.dtype == np.uint16 and u16.max() == 65535 and u16.min() >= 1000
    assert ((u16 >> 8) != 0).all() and (u16.astype(np.uint8) != u16).all()
    assert f64.dtype == np.float64 and (f64.astype(np.float32).astype(np.float64) != f64).all()
    # cast, then normalize: normalizing in float64 first gives another float32 map
    v = f64 - f64.min()
    assert not np.array_equal((v / v.max()).astype(np.float32), IC.read_data_ref(f64, {}))


def test_make_cfg_refuses_negative_channel_end():
    """slice(channel_begin, -1) drops the last channel; in the struct -1 encodes None."""
    for ce in (-1, -2):
        with pytest.raises(ValueError, match='channel_end'):
            _abi.make_cfg({'channel_end': ce}, IC.BLOCK_SHAPE)
    with pytest.raises(ValueError, match='channel_end'):
        O.ws_blocks({'channel_end': -1}, IC.BLOCK_SHAPE, [dict(input=IC.block_4d('uint8'))])
    cfg = _abi.make_cfg({'channel_end': None}, IC.BLOCK_SHAPE)
    assert (cfg.channel_begin, cfg.channel_end) == (0, -1)
    cfg = _abi.make_cfg({}, IC.BLOCK_SHAPE)
    assert (cfg.channel_begin, cfg.channel_end) == (0, -1)
    cfg = _abi.make_cfg({'channel_end': 2}, IC.BLOCK_SHAPE)
    assert (cfg.channel_begin, cfg.channel_end) == (0, 2)
    cfg = _abi.make_cfg({'channel_begin': -3}, IC.BLOCK_SHAPE)
    assert (cfg.channel_begin, cfg.channel_end) == (-3, -1)
    cfg = _abi.make_cfg({'channel_begin': 1, 'channel_end': 0}, IC.BLOCK_SHAPE)
    assert (cfg.channel_begin, cfg.channel_end) == (1, 0)


def test_watershed_task_slices_a_negative_channel_end_on_the_host():
    """The watershed task reads `ds_in[channel_begin:channel_end]` itself (and then hands the
    library `0, None`), so a negative end keeps the reference's meaning there."""
    from cluster_tools_amd.utils.blocking import Blocking
    from cluster_tools_amd.watershed import watershed
    x = IC.block_4d('uint8')
    blocking = Blocking([0, 0, 0], list(IC.SHAPE_4D), list(IC.SHAPE_4D))
    b = watershed._read_block(blocking, 0, x, None, None, dict(channel_begin=1, channel_end=-1), 0)
    np.testing.assert_array_equal(b['input'], x[1:3])
