"""The seed stage from k_localmax's bitmaps: k_localmax stores the member bitmap word and an
"equal" bitmap word per (row, 64-voxel word) and the strict maxima's seed-forest entries, and
k_plateau_flag_eq / k_seed_members_eq visit only the words that hold a plateau voxel.
CTWS_SEED_DENSE=1 (read when a handle is opened) runs k_plateau_flag / k_seed_members over every
class byte as before; CTWS_SEED_TILECC=1 builds the seed components with the tile CC.  All three
must give the same classes and seeds bit for bit, the seeds must be the oracle's, and the whole
block must come out the same.  The `seed_dense` timing says which dispatch ran.

The shapes are the smallest that reach every edge of k_localmax's units (8 rows of one 64-voxel
word column): rows of 63, 64, 65 and 130 voxels (a ragged word, exactly one word, a second word of
one voxel, three words), Y of 7, 8, 9, 20 and 45 (one ragged unit, exactly one, one row into the
second, several with a remainder), 1 to 4 slices for the 2-D watershed and 5 to 9 for the 3-D one.
Contents: smoothed noise (strict maxima only: the equal bitmap stays empty and the member bitmap
and the forest are k_localmax's alone), maps quantised to a few levels without seed smoothing
(most words hold plateau voxels; 2-D: 8-connected plateaus with 4-connected seed components, 3-D:
plateaus rooted at their first voxel in scan order), a slice whose dt is all zero beside slices
that are not (the zero short cut), slices without any boundary (a whole-slice plateau of maxima),
a mask, one call with three blocks of different shapes (the blocks' bitmap and voxel offsets) and
pass-2 blocks with initial seeds.  (Pass 2 relabels its seeds with the initial ids before the stop
after the seed stage, so there the seeds of the dispatches are compared with each other and the
whole block with the oracle's flood model instead of the seeds with the oracle's.)
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from cases import BLOCK_SHAPE
from cluster_tools_amd.synthetic import boundary_map, ellipsoid_mask

pytestmark = pytest.mark.gpu

D3 = dict(apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=(0., 2., 2.), sigma_weights=(0., 2., 2.))
Q2 = dict(sigma_seeds=0.)
Q3 = dict(apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=0., sigma_weights=0.)


def _noise(shape, seed):
    return np.random.RandomState(seed).rand(*shape).astype(np.float32)


def _quant(shape, seed, levels=4):
    return (np.round(boundary_map(shape, seed=seed) * levels) / levels).astype(np.float32)


def _zero_dt_slice(shape, seed, z):
    """slice z all boundary: its dt is all zero, one plateau that is one seed; the zeros of the
    other slices take the short cut"""
    x = boundary_map(shape, seed=seed).copy()
    x[z] = 1.0
    return x


def _sparse(shape):
    """a few boundary voxels: slices without any are whole-slice plateaus of maxima, and the dt of
    the others is equal on every symmetric position (the 2d_sparse_fg construction)"""
    x = np.zeros(shape, np.float32)
    z, y, xx = shape
    x[0, y // 3, xx // 4] = x[0, y - 2, xx - 3] = 1.0
    x[z - 1, :, xx // 2] = 1.0
    return x


def _cases():
    c = {}
    # smoothed noise: strict maxima only
    for z, y, x in ((1, 7, 63), (2, 8, 64), (3, 9, 65), (4, 20, 130), (2, 45, 65)):
        c['smooth2d-%dx%dx%d' % (z, y, x)] = ({}, dict(input=_noise((z, y, x), z * y + x)))
    for z, y, x in ((5, 7, 130), (6, 8, 65), (7, 9, 64), (8, 45, 63), (9, 20, 130)):
        c['smooth3d-%dx%dx%d' % (z, y, x)] = (D3, dict(input=_noise((z, y, x), z * y + x)))
    # quantised maps without seed smoothing: plateaus in most words
    for z, y, x in ((1, 9, 63), (2, 7, 65), (3, 45, 130), (4, 8, 64), (2, 20, 65)):
        c['quant2d-%dx%dx%d' % (z, y, x)] = (Q2, dict(input=_quant((z, y, x), z * y + x)))
    for z, y, x in ((5, 8, 65), (6, 7, 64), (7, 45, 63), (8, 9, 130), (9, 20, 130)):
        c['quant3d-%dx%dx%d' % (z, y, x)] = (Q3, dict(input=_quant((z, y, x), z * y + x)))
    c['quant2d-8levels-3x20x130'] = (Q2, dict(input=_quant((3, 20, 130), 61, 8)))
    c['quant3d-8levels-5x20x65'] = (Q3, dict(input=_quant((5, 20, 65), 62, 8)))
    # a slice with dt = 0 beside slices with dt > 0
    c['zero_slice2d-3x20x65'] = ({}, dict(input=_zero_dt_slice((3, 20, 65), 63, 1)))
    c['zero_slice2d-sigma0-4x9x130'] = (Q2, dict(input=_zero_dt_slice((4, 9, 130), 64, 0)))
    c['zero_slice3d-5x20x65'] = (D3, dict(input=_zero_dt_slice((5, 20, 65), 65, 2)))
    # whole-slice plateaus of maxima
    c['sparse2d-3x20x130'] = ({}, dict(input=_sparse((3, 20, 130))))
    c['sparse2d-sigma0-4x45x65'] = (Q2, dict(input=_sparse((4, 45, 65))))
    c['sparse3d-5x9x64'] = (D3, dict(input=_sparse((5, 9, 64))))
    c['sparse3d-sigma0-6x20x63'] = (Q3, dict(input=_sparse((6, 20, 63))))
    # masks
    c['mask2d-3x45x130'] = ({}, dict(input=boundary_map((3, 45, 130), seed=66), mask=ellipsoid_mask((3, 45, 130))))
    c['mask2d-quant-2x20x65'] = (Q2, dict(input=_quant((2, 20, 65), 67), mask=ellipsoid_mask((2, 20, 65))))
    c['mask3d-quant-7x20x65'] = (Q3, dict(input=_quant((7, 20, 65), 68), mask=ellipsoid_mask((7, 20, 65))))
    return c


CASES = _cases()

# three blocks of different shapes in one call
BATCHES = {
    'batch2d': (Q2, [dict(input=_quant((2, 9, 65), 71)), dict(input=_noise((4, 20, 130), 72)),
                     dict(input=_quant((1, 45, 63), 73))]),
    'batch2d-smooth': ({}, [dict(input=_noise((3, 7, 64), 74)), dict(input=_sparse((2, 20, 130))),
                            dict(input=_quant((4, 9, 65), 75))]),
    'batch3d': (Q3, [dict(input=_quant((5, 9, 65), 76)), dict(input=_noise((9, 20, 130), 77)),
                     dict(input=_quant((6, 45, 63), 78))]),
}


def _pass2_block(shape, seed, quant):
    """initial seeds as pass 1 leaves them in a pass-2 block's halo: ids on two faces"""
    x = _quant(shape, seed) if quant else boundary_map(shape, seed=seed)
    init = np.zeros(shape, np.uint64)
    init[:, :3, :] = 7001
    init[:, 3:, :2] = 7002
    init[:, shape[1] - 2:, 40:] = 7003
    return dict(input=x, initial_seeds=init)


PASS2 = {
    'pass2-2d-3x20x65': ({}, _pass2_block((3, 20, 65), 81, False)),
    'pass2-2d-quant-2x45x130': (Q2, _pass2_block((2, 45, 130), 82, True)),
    'pass2-3d-7x20x65': (D3, _pass2_block((7, 20, 65), 83, False)),
    'pass2-3d-quant-5x9x130': (Q3, _pass2_block((5, 9, 130), 84, True)),
}

TILECC = ['quant2d-3x45x130', 'quant3d-9x20x130', 'smooth2d-4x20x130', 'smooth3d-8x45x63', 'sparse2d-3x20x130',
          'sparse3d-sigma0-6x20x63', 'zero_slice2d-3x20x65', 'mask3d-quant-7x20x65']


def _handle(env):
    from cluster_tools_amd import ctws
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ctws.Handle(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope='module')
def dense_handle():
    h = _handle({'CTWS_SEED_DENSE': '1'})
    yield h
    h.close()


@pytest.fixture(scope='module')
def tilecc_handle():
    h = _handle({'CTWS_SEED_TILECC': '1'})
    yield h
    h.close()


def _oracle_seeds(config, dt):
    if not config.get('apply_ws_2d', True):
        return O.make_seeds(dt, config)
    out = np.zeros(dt.shape, np.uint32)
    n = 0
    for z in range(dt.shape[0]):
        s = O.make_seeds(dt[z], config)
        s[s > 0] += n
        n = max(n, int(s.max()))
        out[z] = s
    return out


def _classes(config, sm, dt):
    """k_localmax's classes restated: bit 0 a neighbour is greater, bit 1 a neighbour is equal
    (8 in-plane neighbours for the 2-D watershed, 6 for the 3-D one); a zero of a slice (2-D) /
    block (3-D) whose dt has a positive value counts as below a neighbour and not as equal"""
    ws2 = config.get('apply_ws_2d', True)
    Z, Y, X = sm.shape
    p = np.pad(sm, 1, constant_values=-np.inf)
    if ws2:
        offs = [(0, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
        pos = dt.reshape(Z, -1).max(axis=1)[:, None, None] > 0
    else:
        offs = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
        pos = dt.max() > 0
    gt = np.zeros(sm.shape, bool)
    eq = np.zeros(sm.shape, bool)
    for dz, dy, dx in offs:
        n = p[1 + dz:1 + dz + Z, 1 + dy:1 + dy + Y, 1 + dx:1 + dx + X]
        gt |= n > sm
        eq |= n == sm
    zero = (sm == 0) & pos
    gt[zero] = True
    eq[zero] = False
    return gt.astype(np.uint8) | (eq.astype(np.uint8) << 1)


def _smoothed(config):
    s = config.get('sigma_seeds', 2.0)
    return any(s) if isinstance(s, (tuple, list)) else bool(s)


def _numbered(blocks):
    return [dict(b, block_id=3 + k) for k, b in enumerate(blocks)]


def _seed_stage(h, config, blocks, pass_id=0):
    """-> per block, after the seed stage: (seed labels, the `cls` bytes -- by then the flood's
    fixed flags of the seeds, written over the classes --, seed map, dt)"""
    h.debug_set_stop(1)
    try:
        h.ws_blocks(config, BLOCK_SHAPE, _numbered(blocks), pass_id=pass_id)
        return [(h.debug_read('labels', k, b['input'].shape) & np.uint32(0x7FFFFFFF),
                 h.debug_read('cls', k, b['input'].shape),
                 h.debug_read('seedmap' if _smoothed(config) else 'dt', k, b['input'].shape),
                 h.debug_read('dt', k, b['input'].shape)) for k, b in enumerate(blocks)]
    finally:
        h.debug_set_stop(0)


def _whole(h, config, blocks, pass_id=0):
    return h.ws_blocks(config, BLOCK_SHAPE, _numbered(blocks), pass_id=pass_id), h.timings()


def _assert_same(h_new, h_old, config, blocks, dense_old, pass_id=0, oracle_seeds=True):
    new = _seed_stage(h_new, config, blocks, pass_id)
    old = _seed_stage(h_old, config, blocks, pass_id)
    for (ln, cn, _, _), (lo, co, _, _) in zip(new, old):
        np.testing.assert_array_equal(ln, lo)
        np.testing.assert_array_equal(cn, co)
    if oracle_seeds:
        refs = O.ws_blocks(config, BLOCK_SHAPE, _numbered(blocks), with_stages=True)
        for (ln, _, _, _), ref in zip(new, refs):
            np.testing.assert_array_equal(ln, _oracle_seeds(config, ref['dt']))
    rn, tn = _whole(h_new, config, blocks, pass_id)
    ro, to = _whole(h_old, config, blocks, pass_id)
    # (a batch that runs again, as pass-2 blocks with a hint do, counts again)
    assert tn['seed_dense'] == 0 and (to['seed_dense'] > 0) == dense_old, (tn, to)
    for a, b in zip(rn, ro):
        assert a['status'] == b['status'] == 0
        np.testing.assert_array_equal(a['output'], b['output'])
        assert (a['max_label'], a['n_ids']) == (b['max_label'], b['n_ids'])
    return rn


@pytest.mark.parametrize('name', sorted(CASES))
def test_bitmap_equals_dense(gpu_handle, dense_handle, name):
    config, block = CASES[name]
    _assert_same(gpu_handle, dense_handle, config, [block], True)


@pytest.mark.parametrize('name', sorted(BATCHES))
def test_bitmap_equals_dense_three_blocks(gpu_handle, dense_handle, name):
    config, blocks = BATCHES[name]
    _assert_same(gpu_handle, dense_handle, config, blocks, True)


@pytest.mark.parametrize('name', sorted(PASS2))
def test_bitmap_equals_dense_pass2(gpu_handle, dense_handle, name):
    config, block = PASS2[name]
    res = _assert_same(gpu_handle, dense_handle, config, [block], True, pass_id=1, oracle_seeds=False)
    with O.flood_model():
        ref = O.ws_blocks(config, BLOCK_SHAPE, _numbered([block]), pass_id=1)[0]
    assert ref['status'] == 0
    np.testing.assert_array_equal(res[0]['output'], ref['output'])


@pytest.mark.parametrize('name', TILECC)
def test_tilecc_equals_bitmap(gpu_handle, tilecc_handle, name):
    config, block = CASES[name]
    _assert_same(gpu_handle, tilecc_handle, config, [block], True, oracle_seeds=False)


def test_cases_reach_both_kinds_of_words(gpu_handle):
    """The classes restated on the GPU's seed maps: the smoothed-noise cases have no plateau voxel
    at all (every word is k_localmax's); every quantised case has plateau voxels with and without
    a greater neighbour, and some of them words without a plateau voxel too."""
    mixed = 0
    for name in sorted(CASES):
        config, block = CASES[name]
        _, _, sm, dt = _seed_stage(gpu_handle, config, [block])[0]
        cls = _classes(config, sm, dt)
        if name.startswith('smooth'):
            assert not (cls & 2).any() and (cls == 0).any(), name
        if name.startswith('quant'):
            assert (cls == 2).any() and (cls == 3).any(), name
            pad = (-cls.shape[2]) % 64
            eq = np.pad(cls & 2, ((0, 0), (0, 0), (0, pad))).reshape(cls.shape[0], cls.shape[1], -1, 64).any(axis=3)
            mixed += bool(eq.any() and not eq.all())
    assert mixed >= 4
