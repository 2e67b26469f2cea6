"""The first flood's fixpoint check that also counts the labels (k_flood_verify_hist2d) and the
size filter's plan over many workgroups (k_sf_plan).

2-D ws, pass 1, packed keys: the check of the first flood counts the labels of every unit's centre
rows into the size filter's histogram, and k_hist2d is not launched.  CTWS_FUSE_HIST=0 (read when
a handle is opened) launches k_flood_verify + k_hist2d as before.  Both handles must give the same
blocks and the same size-filter plan (the `sf_sparse_blocks`, `sf_redo_blocks` and
`auto_seeded_blocks` timings, which k_sf_plan and the counts decide), and the flood model's blocks
bit for bit.  The `hist_fused` timing says which kernels ran.  conftest.py sets CTWS_VERIFY=2: a
violation of the fixpoint is an error in every run here.

The shapes are the smallest at which the pieces can go wrong: rows of 63, 64, 65 and 130 voxels
(a ragged word, exactly one word, a second word of one voxel, three words), Y of 20, 37 and 45
(not a multiple of the unit's 4 rows; fewer units than the workgroup has waves), Z of 1 and 3, a
slice whose segments are all below the size filter, a slice that is one label, a masked block, a
cropped block, every input dtype, a slice with more labels than the host-sized LDS histogram
of its batch, and a slice with more labels than the largest LDS histogram (kHist2dBins).
k_sf_plan: a block of 80 slices (the workgroup that decides marks the slices' survivors with all
of its waves, 64 slices per wave), and blocks of more than 4096 labels (kSfPlanLabels: several
workgroups per block) in 2-D with 20 slices (the slices strided over 4 workgroups x 4 waves) and
in 3-D, once sparse and once with too many small segments for the walk (both from the summed
counts of two workgroups).
(A slice without any seed cannot be built: a slice that is all boundary has dt = 0 everywhere, one
plateau, which is one seed.  The auto-seeded regrow is reached through the size filter instead.)
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from cases import BLOCK_SHAPE, mixed_regrow_plans
from cluster_tools_amd.synthetic import boundary_map, ellipsoid_mask

pytestmark = pytest.mark.gpu

D3 = dict(apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=(0., 2., 2.), sigma_weights=(0., 2., 2.))
HIST2D_BINS = 8192  # kHist2dBins (ctws_kernels.h)


def _bm(shape, seed, dtype='float32'):
    x = boundary_map(shape, seed=seed)
    if dtype == 'float32':
        return x
    if dtype == 'float64':
        return x.astype(np.float64)
    return np.round(x * np.iinfo(dtype).max).astype(dtype)


def _noise(shape, seed):
    return np.random.RandomState(seed).rand(*shape).astype(np.float32)


def _noise_slices():
    """slice 0 pure noise (with size_filter 400 every segment of it is removed: its regrow is
    auto-seeded), slices 1 and 2 regular"""
    x = _bm((3, 45, 65), 31).copy()
    x[0] = _noise((45, 65), 32)
    return x


def _boundary_slice():
    """slice 1 all boundary: dt = 0 there, one plateau, so the slice's label range is one label"""
    x = _bm((3, 37, 130), 33).copy()
    x[1] = 1.0
    return x


def _skewed_slices():
    """slice 0 noise, slices 1 to 3 regular: without seed smoothing 1012 labels in slice 0 and
    about 30 in each of the others, so the LDS histogram, which the host sizes to the block's
    labels per slice (512 bins here), is too small for slice 0 alone"""
    x = _bm((4, 64, 130), 44).copy()
    x[0] = _noise((64, 130), 45)
    return x


def _cases():
    x4 = np.stack([_bm((3, 37, 65), s) for s in (41, 42, 43)])
    c = {
        'x63-3x37': ({}, dict(input=_bm((3, 37, 63), 21))),
        'x64-1x20': ({}, dict(input=_bm((1, 20, 64), 22))),
        'x65-3x45': ({}, dict(input=_bm((3, 45, 65), 23))),
        'x130-3x37': ({}, dict(input=_bm((3, 37, 130), 24))),
        'x130-1x45-sf5': (dict(size_filter=5, sigma_seeds=1.0), dict(input=_bm((1, 45, 130), 25))),
        'noise_slice-sf400': (dict(size_filter=400), dict(input=_noise_slices())),
        'all_small-sf1e9': (dict(size_filter=10 ** 9), dict(input=_bm((3, 37, 65), 26))),
        'boundary_slice': ({}, dict(input=_boundary_slice())),
        'mask': ({}, dict(input=_bm((3, 45, 130), 27), mask=ellipsoid_mask((3, 45, 130)))),
        'halo_crop': (dict(halo=[0, 8, 8]), dict(input=_bm((3, 45, 130), 28), inner_begin=(0, 8, 8),
                                                 inner_shape=(3, 29, 114), crop_relabel=True)),
        '3d-5x20x70': (D3, dict(input=_bm((5, 20, 70), 29))),
        'u8': ({}, dict(input=_bm((3, 37, 65), 34, 'uint8'))),
        'u16-invert': (dict(invert_inputs=True, threshold=.3), dict(input=_bm((3, 37, 65), 35, 'uint16'))),
        'f64': ({}, dict(input=_bm((3, 37, 65), 36, 'float64'))),
        'f32-invert': (dict(invert_inputs=True, threshold=.3), dict(input=_bm((3, 37, 65), 37))),
        '4d-channels': (dict(agglomerate_channels='max', channel_begin=1), dict(input=x4)),
        'sigmas-differ': (dict(sigma_seeds=1.0, sigma_weights=2.0), dict(input=_bm((3, 37, 65), 38))),
        'sigma_weights0': (dict(sigma_weights=0.), dict(input=_bm((3, 37, 65), 39))),
        'skewed_slices-4x64x130': (dict(sigma_seeds=0., threshold=.2), dict(input=_skewed_slices())),
        'deep-80x20x65': (dict(size_filter=25), dict(input=_bm((80, 20, 65), 51))),
        'deep-80x20x65-sf10': (dict(size_filter=10, sigma_seeds=1.0), dict(input=_bm((80, 20, 65), 51))),
        'noise-20x48x130-sf3': (dict(size_filter=3, sigma_seeds=0., threshold=.2),
                                dict(input=_noise((20, 48, 130), 52))),
        '3d-noise-8x64x130-sf3': (dict(D3, size_filter=3, sigma_seeds=0., threshold=.2),
                                  dict(input=_noise((8, 64, 130), 53))),
        '3d-noise-8x64x130-sf64': (dict(D3, size_filter=64, sigma_seeds=0., threshold=.2),
                                   dict(input=_noise((8, 64, 130), 53))),
        # noise without seed smoothing: every strict maximum of the dt is a seed (see
        # test_many_labels_slice_exceeds_bins)
        'many_labels-1x256x320': (dict(sigma_seeds=0., threshold=.2), dict(input=_noise((1, 256, 320), 40))),
    }
    return c


CASES = _cases()
# the 3-D flood keeps k_flood_verify<3> + k_hist
FUSED = {n: 0 if n.startswith('3d') else 1 for n in CASES}
PLAN = ('sf_sparse_blocks', 'sf_redo_blocks', 'auto_seeded_blocks')


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
def two_kernel_handle():
    h = _handle({'CTWS_FUSE_HIST': '0'})
    yield h
    h.close()


_MODEL = {}


def _model(name):
    if name not in _MODEL:
        config, block = CASES[name]
        with O.flood_model():
            _MODEL[name] = O.ws_blocks(config, BLOCK_SHAPE, [dict(block, block_id=3)])[0]
    return _MODEL[name]


def _run(h, name):
    config, block = CASES[name]
    res = h.ws_blocks(config, BLOCK_SHAPE, [dict(block, block_id=3)])[0]
    return res, h.timings()


@pytest.mark.parametrize('name', sorted(CASES))
def test_fused_equals_two_kernels(gpu_handle, two_kernel_handle, name):
    new, tn = _run(gpu_handle, name)
    old, to = _run(two_kernel_handle, name)
    assert (tn['hist_fused'], to['hist_fused']) == (FUSED[name], 0), (tn, to)
    assert new['status'] == old['status']
    np.testing.assert_array_equal(new['output'], old['output'])
    assert (new['max_label'], new['n_ids']) == (old['max_label'], old['n_ids'])
    assert [tn[k] for k in PLAN] == [to[k] for k in PLAN], (tn, to)


@pytest.mark.parametrize('name', sorted(CASES))
def test_fused_matches_model(gpu_handle, name):
    ref = _model(name)
    res, tm = _run(gpu_handle, name)
    assert tm['hist_fused'] == FUSED[name], tm
    assert res['status'] == ref['status'] == 0
    np.testing.assert_array_equal(res['output'], ref['output'])
    assert res['max_label'] == ref['max_label']


def test_plans_cover_sparse_and_auto_seeded(gpu_handle):
    """The cases reach both outcomes of k_sf_plan and the auto-seeded regrow."""
    assert _run(gpu_handle, 'x130-1x45-sf5')[1]['sf_sparse_blocks'] == 1
    for name in ('noise_slice-sf400', 'all_small-sf1e9'):
        tm = _run(gpu_handle, name)[1]
        assert (tm['sf_sparse_blocks'], tm['auto_seeded_blocks']) == (0, 1), (name, tm)


# name -> (k_sf_plan's workgroups per block: labels // kSfPlanLabels + 1, sparse, auto-seeded)
PLANNED = {'deep-80x20x65': (1, 1, 0), 'deep-80x20x65-sf10': (1, 1, 0), 'noise-20x48x130-sf3': (4, 1, 0),
           '3d-noise-8x64x130-sf3': (2, 1, 0), '3d-noise-8x64x130-sf64': (2, 0, 0)}
_RAW = {}


def _raw_labels(name):
    """the flood's labels: the ids of the model's block without the size filter"""
    if name not in _RAW:
        config, block = CASES[name]
        with O.flood_model():
            _RAW[name] = O.ws_blocks(dict(config, size_filter=0), BLOCK_SHAPE, [dict(block, block_id=3)])[0]
        assert _RAW[name]['status'] == 0
    return _RAW[name]['output']


@pytest.mark.parametrize('name', sorted(PLANNED))
def test_plan_of_deep_and_many_label_blocks(gpu_handle, name):
    """k_sf_plan's decision against its conditions restated on the model's unfiltered block
    (cases.mixed_regrow_plans), on blocks whose plan takes several workgroups or marks more
    slices than one wave holds; the label counts that choose the grid are checked too."""
    config, block = CASES[name]
    split, sparse, auto = PLANNED[name]
    assert np.unique(_raw_labels(name)).size // 4096 + 1 == split
    (cpu_sparse, nsmall), = mixed_regrow_plans(config, [dict(block, block_id=3)])
    assert cpu_sparse == bool(sparse) and nsmall > 0
    tm = _run(gpu_handle, name)[1]
    assert (tm['sf_sparse_blocks'], tm['sf_redo_blocks'], tm['auto_seeded_blocks']) == (sparse, 0, auto), tm


def test_skewed_slice_exceeds_host_bins():
    """Slice 0 of the skewed block has more labels than the LDS bins the host gives its batch (the
    power of two, from 512, above 1.5 x the block's labels per slice), and fewer than kHist2dBins."""
    per = [np.unique(p).size for p in _raw_labels('skewed_slices-4x64x130')]
    per_slice = sum(per) // len(per) + 1
    bins = 512
    while bins < HIST2D_BINS and bins < per_slice + per_slice // 2:
        bins *= 2
    assert bins < per[0] < HIST2D_BINS and max(per[1:]) < bins, (per, bins)


def test_channel_range_keeps_generic_prep(gpu_handle):
    """A 4-D input with a channel range runs the generic normalize / x-pass kernel."""
    assert int(_run(gpu_handle, '4d-channels')[1]['prep_kernel']) == 0


def test_many_labels_slice_exceeds_bins():
    """The many-labels slice has more labels than k_flood_verify_hist2d's largest LDS histogram,
    so it counts with global atomics (the unfiltered model's ids are the flood's labels: 9756)."""
    assert np.unique(_raw_labels('many_labels-1x256x320')).size > HIST2D_BINS

