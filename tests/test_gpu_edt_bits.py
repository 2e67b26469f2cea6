"""The EDT y pass fed by the x pass's per-word records (k_prep_edt_x_co<.., BITS>, k_edt_col_bits).

Typed batches on the integer EDT hand the rows' foreground bits to the y pass, which computes the
squared x distances itself; CTWS_EDT_BITS=0 (read when a handle is opened) keeps the per-voxel
g2 array and k_edt_col for every batch.  Both must give the oracle's dt bit for bit.  The
inputs are hand-built around what the records encode: the first and last bit of a row, a word
boundary, empty words between two foreground voxels, rows and slices without foreground, and
columns whose distances sit on the bounded search's cap (kEdtSearchCap = 48) or go to the
lower-envelope pass (k_edt_col_fh), which at Y = 130 and 200 also lie across the windows of the
y pass's row ring.
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from cases import make_cases, BLOCK_SHAPE
from cluster_tools_amd.synthetic import ellipsoid_mask

pytestmark = pytest.mark.gpu

# the non-final y pass (3-D dt).  The volumes are 1 to 3 slices deep, so z is not smoothed (the
# default sigma = 2 needs 7 voxels along every smoothed axis); dt does not depend on the sigmas
D3 = dict(apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=(0., 2., 2.), sigma_weights=(0., 2., 2.))


@pytest.fixture(scope='module', params=['bits', 'old'])
def edt_handle(request):
    from cluster_tools_amd import ctws
    env = {'CTWS_EDT_BITS': '0'} if request.param == 'old' else {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h = ctws.Handle(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield h
    h.close()


@pytest.fixture(scope='module')
def old_handle():
    from cluster_tools_amd import ctws
    saved = os.environ.get('CTWS_EDT_BITS')
    os.environ['CTWS_EDT_BITS'] = '0'
    try:
        h = ctws.Handle(0)
    finally:
        if saved is None:
            os.environ.pop('CTWS_EDT_BITS', None)
        else:
            os.environ['CTWS_EDT_BITS'] = saved
    yield h
    h.close()


def _vol(shape):
    return np.zeros(shape, np.float32)


def p_first_bit(shape):
    """one foreground voxel at x = 0 of one row per slice, the slice's other rows empty"""
    v = _vol(shape)
    for z in range(shape[0]):
        v[z, (3 + 5 * z) % shape[1], 0] = 1.0
    return v


def p_last_bit(shape):
    """foreground only at x = X - 1: the last valid bit of a partial word"""
    v = _vol(shape)
    v[:, :, -1] = 1.0
    return v


def p_word_boundary(shape):
    """x = 63 in even rows, x = 64 in odd rows"""
    v = _vol(shape)
    v[:, 0::2, 63] = 1.0
    v[:, 1::2, 64] = 1.0
    return v


def p_row_ends(shape):
    """x = 0 and x = X - 1 only (X = 200: two empty words between them)"""
    v = _vol(shape)
    v[:, :, 0] = 1.0
    v[:, :, -1] = 1.0
    return v


def p_edge_rows(shape):
    """rows 0 and Y - 1 only"""
    v = _vol(shape)
    v[:, 0, :] = 1.0
    v[:, -1, :] = 1.0
    return v


def p_empty_slice(shape):
    """slice 0 without foreground next to slices with some"""
    v = p_random(shape)
    v[0] = 0.0
    return v


def p_random(shape):
    """random foreground of density 1 / 500"""
    rng = np.random.RandomState(1234)
    return (rng.rand(*shape) < 1.0 / 500).astype(np.float32)


S65, S127, S129, S200, S100T, S200T = (2, 9, 65), (2, 70, 127), (1, 130, 129), (3, 40, 200), (1, 100, 64), (1, 200, 64)

# name -> (config, block)
DT_CASES = {}
for _pat, _shapes in ((p_first_bit, (S65, S127, S129, S200T)),
                      (p_last_bit, (S65, S127, S129, S200)),
                      (p_word_boundary, (S65, S127, S129, S200)),
                      (p_row_ends, (S200,)),
                      (p_edge_rows, (S100T, S129, S200T, S200)),
                      (p_empty_slice, (S127, S200)),
                      (p_random, (S65, S127, S129, S200, S100T, S200T))):
    for _s in _shapes:
        DT_CASES['%s-%dx%dx%d' % ((_pat.__name__[2:],) + _s)] = ({}, dict(input=_pat(_s)))
for _pat, _shapes in ((p_word_boundary, (S127, S200)), (p_edge_rows, (S100T, S129, S200T)),
                      (p_random, (S127, S200, S200T))):
    for _s in _shapes:
        DT_CASES['3d-%s-%dx%dx%d' % ((_pat.__name__[2:],) + _s)] = (D3, dict(input=_pat(_s)))
DT_CASES['u8-random-3x40x200'] = ({}, dict(input=(p_random(S200) * 255).astype(np.uint8)))
DT_CASES['mask-random-2x70x127'] = ({}, dict(input=p_random(S127), mask=ellipsoid_mask(S127)))
DT_CASES['3d-mask-word_boundary-3x40x200'] = (D3, dict(input=p_word_boundary(S200), mask=ellipsoid_mask(S200)))

_REF = {}


def _ref_dt(key, config, blocks):
    if key not in _REF:
        _REF[key] = [r['dt'] for r in O.ws_blocks(config, BLOCK_SHAPE, blocks, with_stages=True)]
    return _REF[key]


def _gpu_dt(h, config, blocks):
    h.debug_set_stop(1)
    try:
        h.ws_blocks(config, BLOCK_SHAPE, blocks)
        return [h.debug_read('dt', i, b['input'].shape) for i, b in enumerate(blocks)]
    finally:
        h.debug_set_stop(0)


@pytest.mark.parametrize('name', sorted(DT_CASES))
def test_dt_matches_oracle(edt_handle, name):
    config, block = DT_CASES[name]
    blocks = [dict(block, block_id=3)]
    ref = _ref_dt(name, config, blocks)
    dt = _gpu_dt(edt_handle, config, blocks)
    np.testing.assert_array_equal(dt[0], ref[0])


@pytest.mark.parametrize('config', [{}, D3], ids=['2d', '3d'])
def test_two_shapes_in_one_call(edt_handle, config):
    """Blocks of different shapes in one batch: the grid is sized by the largest block."""
    blocks = [dict(input=p_random((2, 40, 200)), block_id=1), dict(input=p_word_boundary((2, 70, 127)), block_id=2)]
    ref = _ref_dt('two_shapes_%d' % len(config), config, blocks)
    dt = _gpu_dt(edt_handle, config, blocks)
    for g, r in zip(dt, ref):
        np.testing.assert_array_equal(g, r)


CASES = make_cases()
_MODEL = {}


@pytest.mark.parametrize('name', ['2d_default', '3d_default', '2d_sparse_fg', '3d_sparse_fg', '3d_wide512_mask',
                                  '3d_u8', '2d_tall2200'])
def test_old_path_matches_model(old_handle, name):
    """CTWS_EDT_BITS=0: the per-voxel g2 kernels still give the flood model's final labels."""
    config, block = CASES[name]
    if name not in _MODEL:
        with O.flood_model():
            _MODEL[name] = O.ws_blocks(config, BLOCK_SHAPE, [dict(block, block_id=3)])[0]
    ref = _MODEL[name]
    res = old_handle.ws_blocks(config, BLOCK_SHAPE, [dict(block, block_id=3)])[0]
    assert res['status'] == ref['status']
    np.testing.assert_array_equal(res['output'], ref['output'])
