"""GPU: every raw input dtype on every normalize / x-pass kernel path of run_batch.

uint8, uint16 and float64 blocks (tests/input_dtype_cases.py) go through k_input_minmax_t<T> +
k_prep_edt_x_co<4|8|16, T, BITS> (both BITS: the second on a CTWS_EDT_BITS=0 handle), and through
the generic k_input_minmax + k_prep_edt_x with load_raw's dtype switch (4-D inputs with channel
ranges, rows > 1024, blocks of different dtypes in one batch).  Each test asserts the kernel it
means to hit through the `prep_kernel` entry of the handle's timings (include/ctws.h), so that a
change of the dispatch conditions cannot move it onto another kernel unnoticed.

`fin` is compared with read_data_ref, the reference's `_read_data` + `vu.normalize` in numpy, and
fin, dt, hmap, seeds and the final block with the oracle.  Every comparison is array_equal: nothing
here has a tolerance, except the VI of the WatershedFromSeeds outputs to vigra's heap order (0.01,
the project's bar; the flood model's own gap, measured with the oracle, is 0 for the uint16 and
the float64 case).  Further: host staging at element size 2, the device path, WatershedFromSeeds and the
watershed task on a 4-D uint8 n5 input with a negative channel_end."""
import json
import os
import sys

import numpy as np
import pytest

from cluster_tools_amd.metrics import vi_scores
from cluster_tools_amd.synthetic import boundary_map, ellipsoid_mask
from oracle import oracle as O
import input_dtype_cases as IC
from input_dtype_cases import BLOCK_SHAPE, DTYPES
from test_gpu_parity import _oracle_seeds, _oracle_hmap

pytestmark = pytest.mark.gpu

CASES = IC.stage_cases()


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


_STAGES, _MODEL = {}, {}


def _stages(key, config, block):
    """the oracle's stages of one block (computed once, shared, not modified)"""
    if key not in _STAGES:
        _STAGES[key] = O.ws_blocks(config, BLOCK_SHAPE, [dict(block, block_id=3)], with_stages=True)[0]
    return _STAGES[key]


def _model(key, config, blocks):
    """the oracle's final blocks under the flood model (computed once)"""
    if key not in _MODEL:
        with O.flood_model():
            _MODEL[key] = O.ws_blocks(config, BLOCK_SHAPE, blocks)
    return _MODEL[key]


def _gpu_fin(h, config, blocks):
    h.debug_set_stop(1)
    try:
        h.ws_blocks(config, BLOCK_SHAPE, blocks)
        return [h.debug_read('fin', i, np.shape(b['input'])[-3:]) for i, b in enumerate(blocks)]
    finally:
        h.debug_set_stop(0)


def _prep_kernel(h):
    return int(h.timings()['prep_kernel'])


# ---- stages ---------------------------------------------------------------------------------------

# the CTWS_EDT_BITS=0 handle where it changes the kernel
STAGE_PARAMS = [(n, 'bits') for n in sorted(CASES)] + [(n, 'old') for n in sorted(CASES) if CASES[n][2] != CASES[n][3]]


@pytest.mark.parametrize('name,handle', STAGE_PARAMS, ids=['%s-%s' % p for p in STAGE_PARAMS])
def test_stages_bit_exact(gpu_handle, old_handle, name, handle):
    config, block, k_bits, k_old = CASES[name]
    h, kernel = (gpu_handle, k_bits) if handle == 'bits' else (old_handle, k_old)
    ref = _stages(name, config, block)
    shape = ref['input'].shape
    blocks = [dict(block, block_id=3)]
    h.debug_set_stop(1)
    try:
        h.ws_blocks(config, BLOCK_SHAPE, blocks)
        fin = h.debug_read('fin', 0, shape)
        dt = h.debug_read('dt', 0, shape)
        hm = h.debug_read('hmap', 0, shape)
        seeds = h.debug_read('labels', 0, shape) & np.uint32(0x7FFFFFFF)
    finally:
        h.debug_set_stop(0)
    np.testing.assert_array_equal(fin, IC.read_data_ref(block['input'], config, block.get('mask')))
    np.testing.assert_array_equal(fin, ref['input'])
    np.testing.assert_array_equal(dt, ref['dt'])
    np.testing.assert_array_equal(hm, _oracle_hmap(config, ref['input'], ref['dt']))
    np.testing.assert_array_equal(seeds, _oracle_seeds(config, ref['dt']))
    res = h.ws_blocks(config, BLOCK_SHAPE, blocks)[0]
    assert res['status'] == ref['status'] == 0
    assert _prep_kernel(h) == kernel, h.timings()


# ---- the whole block ------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['co16', '4d_range_invert', '4d_min_end3'])
def test_block_matches_model_exactly(gpu_handle, name, dtype):
    config, block, kernel, _ = CASES['%s-%s' % (name, dtype)]
    blocks = [dict(block, block_id=3)]
    ref = _model((name, dtype), config, blocks)[0]
    res = gpu_handle.ws_blocks(config, BLOCK_SHAPE, blocks)[0]
    assert _prep_kernel(gpu_handle) == kernel
    assert res['status'] == ref['status'] == 0
    np.testing.assert_array_equal(res['output'], ref['output'])
    assert res['max_label'] == ref['max_label']


# ---- same values, other type ----------------------------------------------------------------------

def _twins():
    x3, x4 = IC.base_f32(IC.SHAPES_3D['co4'][0]), IC.base_4d()
    cfg4 = IC.CONFIGS_4D['max_begin1']
    u8_3, u8_4 = IC.as_dtype(x3, 'uint8'), IC.as_dtype(x4, 'uint8')
    return {'u16_as_u8-3d': ({}, u8_3.astype(np.uint16), u8_3), 'u16_as_u8-4d': (cfg4, u8_4.astype(np.uint16), u8_4),
            'f64_as_f32-3d': ({}, x3.astype(np.float64), x3), 'f64_as_f32-4d': (cfg4, x4.astype(np.float64), x4)}


TWINS = _twins()


@pytest.mark.parametrize('name', sorted(TWINS))
def test_same_values_in_another_type_give_the_same_result(gpu_handle, name):
    """A uint16 block whose values fit in uint8 against its uint8 twin, a float64 block of float32
    values against its float32 twin: a path cannot merely agree with an oracle sharing its mistake."""
    config, wide, narrow = TWINS[name]
    assert wide.dtype != narrow.dtype and np.array_equal(wide, narrow)
    fw = _gpu_fin(gpu_handle, config, [dict(input=wide, block_id=3)])[0]
    fn = _gpu_fin(gpu_handle, config, [dict(input=narrow, block_id=3)])[0]
    np.testing.assert_array_equal(fw, fn)
    np.testing.assert_array_equal(fw, IC.read_data_ref(narrow, config))
    rw = gpu_handle.ws_blocks(config, BLOCK_SHAPE, [dict(input=wide, block_id=3)])[0]
    rn = gpu_handle.ws_blocks(config, BLOCK_SHAPE, [dict(input=narrow, block_id=3)])[0]
    assert rw['status'] == rn['status'] == 0
    np.testing.assert_array_equal(rw['output'], rn['output'])


# ---- constant and extreme blocks ------------------------------------------------------------------

def _extreme_blocks(dtype):
    shape = IC.SHAPES_3D['co4'][0]
    const = {'uint8': 7, 'uint16': 40000, 'float64': 2.5}[dtype]
    blocks = [dict(input=np.full(shape, const, dtype), block_id=1), dict(input=IC.block_3d('co4', dtype), block_id=2)]
    if dtype == 'uint16':
        rng = np.random.RandomState(3)
        two = np.where(rng.rand(*shape) < .2, 65535, 0).astype(np.uint16)   # only {0, 65535}
        one = np.full(shape, 500, np.uint16)                                # constant but for one voxel
        one[1, 9, 130] = 501
        blocks += [dict(input=two, block_id=3), dict(input=one, block_id=4)]
    return blocks


@pytest.mark.parametrize('dtype', DTYPES)
def test_constant_and_extreme_blocks(gpu_handle, dtype):
    """One batch per dtype: a constant non-zero block (normalized to 0 everywhere: status 2, the
    constant offset), a regular block next to it (the min / max are per block), and for uint16 a
    block of only {0, 65535} and one that is constant except for a single voxel."""
    blocks = _extreme_blocks(dtype)
    ref = _model(('extreme', dtype), {}, blocks)
    res = gpu_handle.ws_blocks({}, BLOCK_SHAPE, blocks)
    assert _prep_kernel(gpu_handle) == 104
    assert ref[0]['status'] == 2 and ref[1]['status'] == 0
    for g, r in zip(res, ref):
        assert g['status'] == r['status']
        np.testing.assert_array_equal(g['output'], r['output'])
    fin = _gpu_fin(gpu_handle, {}, blocks)
    for f, b in zip(fin[1:], blocks[1:]):
        np.testing.assert_array_equal(f, IC.read_data_ref(b['input'], {}))


# ---- blocks of different dtypes in one batch ------------------------------------------------------

def _mixed_blocks():
    return [dict(input=IC.block_3d('co4', 'uint8'), block_id=1), dict(input=IC.block_3d('co8', 'uint16'), block_id=2),
            dict(input=IC.base_f32(IC.SHAPE_REG), block_id=3), dict(input=IC.block_3d('co16', 'float64'), block_id=4)]


def test_mixed_dtype_batch_equals_single_blocks(gpu_handle):
    """A uint8, a uint16, a float32 and a float64 block of different shapes in one call: the generic
    kernels with load_raw's per-block dtype.  Each equals its single-block (typed kernel) result."""
    blocks = _mixed_blocks()
    together = gpu_handle.ws_blocks({}, BLOCK_SHAPE, blocks)
    assert _prep_kernel(gpu_handle) == 0
    for b, t in zip(blocks, together):
        single = gpu_handle.ws_blocks({}, BLOCK_SHAPE, [b])[0]
        assert _prep_kernel(gpu_handle) > 0
        assert single['status'] == t['status'] == 0
        np.testing.assert_array_equal(single['output'], t['output'])
    for f, b in zip(_gpu_fin(gpu_handle, {}, blocks), blocks):
        np.testing.assert_array_equal(f, IC.read_data_ref(b['input'], {}))


# ---- host staging at element size 2 ---------------------------------------------------------------

def test_host_staging_uint16_odd_sizes(gpu_handle):
    """Three uint16 blocks of odd voxel counts, each with a mask, in one host call: the staged
    offsets are 256-aligned, so the inputs' byte sizes (2 N) and the offsets of the inputs and
    masks after them must be kept per element size."""
    shapes = [(3, 9, 67), (3, 11, 65), (5, 7, 69)]
    assert all(np.prod(s) % 2 == 1 for s in shapes)
    blocks = [dict(input=IC.as_dtype(boundary_map(s, seed=30 + i, pitch=(8, 8, 8)), 'uint16'), mask=ellipsoid_mask(s),
                   block_id=i + 1) for i, s in enumerate(shapes)]
    together = gpu_handle.ws_blocks({}, BLOCK_SHAPE, blocks)
    assert gpu_handle.timings()['host_batches'] == 1
    ref = _model('staging', {}, blocks)
    for b, t, r in zip(blocks, together, ref):
        single = gpu_handle.ws_blocks({}, BLOCK_SHAPE, [b])[0]
        assert single['status'] == t['status'] == r['status'] == 0
        np.testing.assert_array_equal(single['output'], t['output'])
        np.testing.assert_array_equal(t['output'], r['output'])
    for f, b in zip(_gpu_fin(gpu_handle, {}, blocks), blocks):
        np.testing.assert_array_equal(f, IC.read_data_ref(b['input'], {}, b['mask']))


# ---- device path ----------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['co8', '4d_range_invert'])
def test_device_path_matches_host_path(gpu_handle, name, dtype):
    import torch
    config, block, kernel, _ = CASES['%s-%s' % (name, dtype)]
    x = np.ascontiguousarray(block['input'])
    host = gpu_handle.ws_blocks(config, BLOCK_SHAPE, [dict(input=x, block_id=2)])[0]
    inp = torch.from_numpy(x).cuda()
    assert str(inp.dtype) == 'torch.' + dtype
    out = torch.zeros(x.shape[-3:], dtype=torch.int64, device='cuda')
    st = gpu_handle.ws_blocks_device(config, BLOCK_SHAPE, [dict(input=inp, output=out, block_id=2)])
    assert _prep_kernel(gpu_handle) == kernel
    assert st[0][0] == host['status'] == 0
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64), host['output'])


# ---- WatershedFromSeeds ---------------------------------------------------------------------------

FS_SHAPE = (6, 20, 200)


def _from_seeds_cases():
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(9)

    def smooth(shape, seed):
        return gaussian_filter(boundary_map(shape, seed=seed), 1.0).astype(np.float32)

    def points(shape):
        s = np.zeros(shape, np.uint64)
        idx = rng.choice(int(np.prod(shape)), 40, replace=False)
        s.flat[idx] = rng.permutation(np.arange(1, 5000))[:40].astype(np.uint64)
        return s

    x = smooth(FS_SHAPE, 11)
    x4 = np.stack([smooth(IC.SHAPE_4D, s) for s in (4, 5, 6, 7)])
    # name -> (config, block, prep_kernel: the typed kernel without the y pass's bits, or the generic one)
    return {'uint16': (dict(size_filter=10), dict(input=IC.as_dtype(x, 'uint16'), seeds=points(FS_SHAPE)), 4),
            'float64': (dict(size_filter=10), dict(input=IC.as_dtype(x, 'float64'), seeds=points(FS_SHAPE)), 4),
            '4d_uint8_end3': (dict(size_filter=10, channel_begin=1, channel_end=3),
                              dict(input=IC.as_dtype(x4, 'uint8'), seeds=points(IC.SHAPE_4D)), 0)}


FS_CASES = _from_seeds_cases()


@pytest.mark.parametrize('name', sorted(FS_CASES))
def test_from_seeds_matches_oracle(gpu_handle, name):
    config, block, kernel = FS_CASES[name]
    with O.flood_model():
        model = O.ws_from_seeds(config, [block])[0]
    heap = O.ws_from_seeds(config, [block])[0]
    res = gpu_handle.ws_from_seeds(config, [block])[0]
    assert _prep_kernel(gpu_handle) == kernel
    assert res['status'] == model['status'] == 0
    np.testing.assert_array_equal(res['output'], model['output'])
    vi = sum(vi_scores(res['output'], heap['output']))
    print('%s: VI to the heap order %.2e' % (name, vi))
    if name != '4d_uint8_end3':
        # (241-level uint8 is tie-dominated, as tests/test_from_seeds_gpu.py's uint8 case: the gap to
        # the heap order is the model's own, 0.33 measured with the oracle, which the equality
        # above already pins)
        assert vi <= 0.01
    assert set(np.unique(res['output'])) - {0} <= set(np.unique(block['seeds'])) - {0}


# ---- the watershed task on a 4-D uint8 n5 input with a negative channel_end -----------------------

def test_watershed_task_negative_channel_end(tmp_path):
    """WatershedLocal with channel_begin=1, channel_end=-1 on a (4, 20, 96, 80) uint8 dataset,
    blocks of [10, 48, 40] without halo: the task slices the channels on the host, where the
    negative end has the reference's meaning (channels 1 and 2), and equals the oracle block by
    block under the flood model."""
    from conftest import luigi_build
    from cluster_tools_amd.utils import volume_utils as vu
    from cluster_tools_amd.utils.blocking import Blocking
    from cluster_tools_amd.watershed.watershed import WatershedLocal
    sh, bs = (20, 96, 80), [10, 48, 40]
    x = IC.as_dtype(np.stack([boundary_map(sh, seed=s) for s in (4, 5, 6, 7)]), 'uint8')
    path = str(tmp_path / 'data.n5')
    with vu.file_reader(path) as f:
        f.create_dataset('affs', data=x, chunks=(1, 10, 48, 40))
    cfg_dir = tmp_path / 'configs'
    cfg_dir.mkdir()
    g = WatershedLocal.default_global_config()
    g.update({'shebang': '#! ' + sys.executable, 'block_shape': bs})
    (cfg_dir / 'global.config').write_text(json.dumps(g))
    c = WatershedLocal.default_task_config()
    c.update(channel_begin=1, channel_end=-1)
    (cfg_dir / 'watershed.config').write_text(json.dumps(c))
    t = WatershedLocal(input_path=path, input_key='affs', output_path=path, output_key='ws',
                       config_dir=str(cfg_dir), tmp_folder=str(tmp_path / 'tmp'), max_jobs=2)
    luigi_build(t, tmp_path / 'tmp')
    with vu.file_reader(path, 'r') as f:
        res = f['ws'][:]
    blocking = Blocking([0, 0, 0], list(sh), bs)
    ref = np.zeros(sh, np.uint64)
    oc = dict(c, channel_begin=0, channel_end=None)    # the oracle gets the sliced channels
    with O.flood_model():
        for bid in range(blocking.numberOfBlocks):
            bb = vu.block_to_bb(blocking.getBlock(bid))
            r = O.ws_blocks(oc, bs, [dict(input=x[(slice(1, -1),) + bb], block_id=bid)])[0]
            assert r['status'] == 0
            ref[bb] = r['output']
    np.testing.assert_array_equal(res, ref)
    # with every channel (what the library took -1 for) the result differs
    with O.flood_model():
        bb = vu.block_to_bb(blocking.getBlock(0))
        every = O.ws_blocks(oc, bs, [dict(input=x[(slice(1, None),) + bb], block_id=0)])[0]['output']
    assert not np.array_equal(every, ref[bb])
