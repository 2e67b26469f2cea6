"""Handle.region_centers / _boxes / _boxes_device (k_regcenter.hip) against the numpy restatement
(tests/region_centers_ref.py), exactly: the smallest shapes at which each mechanism can fail.  Boxes
of at most Handle.REGION_CENTERS_SMALL_VOXELS voxels take the LDS kernel, larger ones the separable
passes through scratch memory; the timings say which ran.  Boxes of the larger path hold few
background voxels or are thin, so that the brute-force restatement stays cheap."""
import numpy as np
import pytest

import region_centers_ref as R
from test_region_centers_ref import load_golden

pytestmark = pytest.mark.gpu

RESOLUTIONS = [(1, 1, 1), (10, 1, 1), (1, 1, 10), (2, 3, 5)]
SMALL = 10000


def _check(h, boxes, resolution=(1, 1, 1), small=None, large=None):
    """boolean boxes as crops of id 7 on a background of 3 -> the centres, checked."""
    crops = [np.where(b, np.uint64(7), np.uint64(3)) for b in boxes]
    ids = [7] * len(crops)
    got_c, got_f = h.region_centers(crops, ids, resolution)
    t = h.timings()
    want_c, want_f = R.centers_for_crops(crops, ids, resolution)
    assert got_c.dtype == np.int64 and got_c.shape == (len(boxes), 3) and got_f.dtype == bool
    np.testing.assert_array_equal(got_f, want_f)
    np.testing.assert_array_equal(got_c, want_c)
    if small is not None:
        assert t['rc_small_objects'] == small, t
    if large is not None:
        assert t['rc_large_objects'] == large, t
    return got_c


def _with_holes(shape, n_holes, seed):
    rng = np.random.RandomState(seed)
    box = np.ones(shape, dtype=bool)
    box.flat[rng.choice(box.size, n_holes, replace=False)] = False
    return box


def test_tiny_boxes(gpu_handle):
    one = np.ones((1, 1, 1), dtype=bool)
    two = np.ones((1, 1, 2), dtype=bool)
    half = np.array([[[True, False]]])
    flip = np.array([[[False, True]]])
    none = np.zeros((1, 1, 2), dtype=bool)
    got = _check(gpu_handle, [one, two, half, flip, none, ~one], small=6, large=0)
    assert got.tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0]]


@pytest.mark.parametrize('resolution', RESOLUTIONS)
def test_word_ends_in_x(gpu_handle, resolution):
    """x extents around the wave's 64 lanes: with ny = nz = 2 (the LDS kernel) and as boxes of the
    larger path, whose x pass walks a row in words of 64 voxels."""
    boxes = []
    for nx in (63, 64, 65, 129):
        for holes in (1, 5):
            boxes.append(_with_holes((2, 2, nx), holes, nx + holes))
    _check(gpu_handle, boxes, resolution, small=len(boxes), large=0)
    boxes = []
    for shape in ((2, 80, 63), (2, 79, 64), (2, 78, 65), (2, 40, 129)):
        assert np.prod(shape) > SMALL
        for holes in (1, 9):
            boxes.append(_with_holes(shape, holes, shape[2] + holes))
    # a hole in the first and in the last word of a row only: the carried positions
    box = np.ones((2, 40, 129), dtype=bool)
    box[:, :, 0] = False
    box[1, 7, 128] = False
    boxes.append(box)
    _check(gpu_handle, boxes, resolution, small=0, large=len(boxes))


@pytest.mark.parametrize('shape', [(3, 4, 5), (3, 60, 70), (40, 30, 11)])
def test_sentinel_through_the_passes(gpu_handle, shape):
    """Rows without background on their line in x, then planes without background in x and y: the
    infinite parabola is carried until a later pass meets background."""
    row = np.ones(shape, dtype=bool)
    row[0, 0, :] = False      # every other row has no background in x
    plane = np.ones(shape, dtype=bool)
    plane[0] = False          # the planes z >= 1 have none in x and y
    column = np.ones(shape, dtype=bool)
    column[:, 0, 0] = False   # background in every plane, in one row each
    last = np.ones(shape, dtype=bool)
    last[-1, -1, :] = False
    n = 4 if np.prod(shape) <= SMALL else 0
    for resolution in ((1, 1, 1), (2, 3, 5)):
        _check(gpu_handle, [row, plane, column, last], resolution, small=n, large=4 - n)


def test_boxes_without_background(gpu_handle):
    shapes = [(1, 1, 1), (1, 1, 2), (3, 1, 1), (2, 3, 4), (5, 5, 5), (1, 7, 3), (1, 1, 300), (10, 10, 100),
              (10, 10, 101), (3, 60, 70), (1, 9000, 2), (9000, 1, 2)]
    for resolution in ((1, 1, 1), (1, 1, 10)):
        got = _check(gpu_handle, [np.ones(s, dtype=bool) for s in shapes], resolution, small=8, large=4)
        assert got.tolist() == [[s[0] - 1, s[1] - 1, s[2] - 1] for s in shapes]


@pytest.mark.parametrize('shape', [(3, 4, 5), (11, 31, 33)])
def test_one_background_voxel_at_each_corner(gpu_handle, shape):
    boxes = []
    for corner in np.ndindex(2, 2, 2):
        box = np.ones(shape, dtype=bool)
        box[tuple(-c for c in corner)] = False  # index 0 or -1 per axis
        boxes.append(box)
    for resolution in RESOLUTIONS:
        _check(gpu_handle, boxes, resolution)


def test_fixture_boxes(gpu_handle):
    kinds, boxes, res, argmax = load_golden()
    crops = [np.where(b, np.uint64(7), np.uint64(3)) for b in boxes]
    for r, want in zip(res, argmax.T):
        got, found = gpu_handle.region_centers(crops, [7] * len(crops), tuple(int(v) for v in r))
        assert found.all()
        flat = [int(np.ravel_multi_index(tuple(c), b.shape)) for c, b in zip(got, boxes)]
        assert flat == [int(w) for w in want], tuple(r)


def test_flat_ties(gpu_handle):
    box = np.ones((1, 4, 4), dtype=bool)
    box[0, 0, 0] = False
    assert _check(gpu_handle, [box]).tolist() == [[0, 3, 3]]
    slab = np.zeros((7, 9, 70), dtype=bool)
    slab[1:-1, 1:-1, 1:-1] = True
    for resolution, want in (((1, 1, 1), (3, 3, 3)), ((10, 1, 1), (1, 4, 4)), ((1, 1, 10), (3, 3, 1))):
        assert _check(gpu_handle, [slab], resolution, small=1).tolist() == [list(want)]
    # the same ties on the larger path: three slabs side by side in one box
    wide = np.zeros((7, 9, 210), dtype=bool)
    for x0 in (0, 70, 140):
        wide[1:-1, 1:-1, x0 + 1:x0 + 69] = True
    for resolution, want in (((1, 1, 1), (3, 3, 3)), ((10, 1, 1), (1, 4, 4)), ((1, 1, 10), (3, 3, 1))):
        assert _check(gpu_handle, [wide], resolution, large=1).tolist() == [list(want)]


def test_the_limit_between_the_two_paths(gpu_handle):
    assert gpu_handle.REGION_CENTERS_SMALL_VOXELS == SMALL
    under = _with_holes((10, 10, 100), 12, 1)
    over = _with_holes((10, 10, 101), 12, 2)
    for resolution in RESOLUTIONS:
        _check(gpu_handle, [under], resolution, small=1, large=0)
        _check(gpu_handle, [over], resolution, small=0, large=1)
        _check(gpu_handle, [over, under, over], resolution, small=1, large=2)


@pytest.mark.parametrize('resolution', [(1, 1, 1), (2, 3, 5)])
def test_column_tiles_of_the_larger_path(gpu_handle, resolution):
    """The y / z passes' tile widths: 64 and narrower (a long line), a partial last tile, and lines
    too long for the LDS, which search in the scratch array."""
    shapes = [(2, 300, 20), (300, 2, 20), (2, 100, 65), (90, 3, 70), (1, 8200, 2), (8200, 1, 2), (1, 2, 8200),
              (3, 4100, 1)]
    boxes = [_with_holes(s, 7, i) for i, s in enumerate(shapes)]
    # denser background in two of them
    rng = np.random.RandomState(3)
    boxes.append(rng.rand(12, 33, 70) < .97)
    boxes.append(rng.rand(2, 300, 20) < .8)
    _check(gpu_handle, boxes, resolution, small=0, large=len(boxes))


def test_mixed_call(gpu_handle):
    """A few hundred objects in one call: both paths, empty boxes, ids absent from their crop."""
    rng = np.random.RandomState(7)
    crops, ids = [], []
    for k in range(300):
        if k % 50 == 10:
            shape = (11, 31, 34)  # the larger path
            crop = np.where(rng.rand(*shape) < .97, 4, rng.randint(0, 4, shape)).astype(np.uint64)
        elif k % 37 == 5:
            shape = [int(s) for s in rng.randint(1, 6, 3)]
            shape[k % 3] = 0      # an empty box
            crop = np.zeros(shape, dtype=np.uint64)
        else:
            shape = tuple(int(s) for s in rng.randint(1, 13, 3))
            crop = rng.randint(0, 5, shape).astype(np.uint64) if k % 3 else np.full(shape, 4, dtype=np.uint64)
        crops.append(crop)
        ids.append(9 if k % 41 == 3 else 4)  # 9 occurs nowhere
    for resolution in ((1, 1, 1), (2, 3, 5)):
        got_c, got_f = gpu_handle.region_centers(crops, ids, resolution)
        t = gpu_handle.timings()
        want_c, want_f = R.centers_for_crops(crops, ids, resolution)
        np.testing.assert_array_equal(got_f, want_f)
        np.testing.assert_array_equal(got_c, want_c)
        assert t['rc_large_objects'] == 6 and t['rc_small_objects'] == 300 - 6 - 8 and t['rc_large_groups'] == 1
        assert 0 < got_f.sum() < 300 and not got_c[~got_f].any()
    got = gpu_handle.region_centers([], [])
    assert got[0].shape == (0, 3) and got[1].shape == (0,)


def test_ids_compare_on_64_bits(gpu_handle):
    lo, mid, hi = 5, 5 + (1 << 32), 5 + (1 << 33)
    rng = np.random.RandomState(9)
    for shape in ((4, 6, 9), (11, 31, 33)):
        crop = rng.choice(np.array([lo, mid, hi, (1 << 63) + 5], dtype=np.uint64), size=shape, p=[.1, .7, .1, .1])
        ids = [lo, mid, hi, (1 << 63) + 5, 1 << 32]
        got_c, got_f = gpu_handle.region_centers([crop] * 5, ids)
        want_c, want_f = R.centers_for_crops([crop] * 5, ids)
        np.testing.assert_array_equal(got_f, want_f)
        np.testing.assert_array_equal(got_c, want_c)
        assert got_f.tolist() == [True, True, True, True, False]
        assert len({tuple(c) for c in got_c[:4]}) > 1


def test_boxes_inside_a_volume_host_and_device(gpu_handle):
    import torch
    rng = np.random.RandomState(4)
    vol = np.kron(rng.randint(0, 6, (4, 5, 6)), np.ones((6, 7, 8), dtype=np.int64)).astype(np.uint64)
    vol[rng.rand(*vol.shape) < .02] = 6
    assert vol.shape == (24, 35, 48)
    boxes, ids = [], []
    for k in range(40):
        b = [int(rng.randint(0, s)) for s in vol.shape]
        e = [int(rng.randint(lo, min(lo + 16, s) + 1)) for lo, s in zip(b, vol.shape)]  # (an extent of 0 occurs)
        boxes.append(b + e)
        ids.append(int(rng.randint(0, 8)))
    boxes.append([0, 0, 0, 24, 35, 48])  # the whole volume and its sprinkled id: the larger path
    ids.append(6)
    boxes = np.array(boxes)
    for resolution in ((1, 1, 1), (5, 1, 1)):
        want_c, want_f = R.centers_for_boxes(vol, ids, boxes, resolution)
        got_c, got_f = gpu_handle.region_centers_boxes(vol, ids, boxes, resolution)
        assert gpu_handle.timings()['rc_large_objects'] >= 1
        np.testing.assert_array_equal(got_f, want_f)
        np.testing.assert_array_equal(got_c, want_c)
        tvol = torch.from_numpy(vol.view(np.int64)).to('cuda:0')
        dev_c, dev_f = gpu_handle.region_centers_boxes_device(tvol, ids, boxes, resolution)
        assert dev_c.is_cuda and dev_c.dtype == torch.int64 and dev_f.dtype == torch.bool
        np.testing.assert_array_equal(dev_c.cpu().numpy(), got_c)
        np.testing.assert_array_equal(dev_f.cpu().numpy(), got_f)
        crops = [vol[b[0]:max(b[0], b[3]), b[1]:max(b[1], b[4]), b[2]:max(b[2], b[5])] for b in boxes]
        packed_c, packed_f = gpu_handle.region_centers(crops, ids, resolution)
        np.testing.assert_array_equal(packed_c, got_c)
        np.testing.assert_array_equal(packed_f, got_f)
    assert 0 < want_f.sum() < len(ids)
    with pytest.raises(ValueError, match='leaves the volume'):
        gpu_handle.region_centers_boxes(vol, [1], [[0, 0, 0, 25, 35, 48]])


def test_refusals(gpu_handle):
    from cluster_tools_amd.ctws import CtwsError
    crop = np.ones((2, 3, 4), dtype=np.uint64)
    for resolution in ((1.5, 1, 1), (0.04, 0.004, 0.004), (1, 1, 1025)):
        with pytest.raises(CtwsError, match=r'\(-5\).*scaled by a common factor.*\[10, 1, 1\]'):
            gpu_handle.region_centers([crop], [1], resolution)
    assert gpu_handle.region_centers([crop], [1], (2.0, 1, 1))[0].tolist() == [[1, 2, 3]]
    # sum((r n)^2) >= 2^31: 46341^2 alone is above, 46340^2 below
    line = np.ones((1, 1, 46341), dtype=np.uint64)
    with pytest.raises(CtwsError, match=r'\(-5\).*object 1 \(id 1\).*2\^31'):
        gpu_handle.region_centers([crop, line], [1, 1])
    with pytest.raises(CtwsError, match=r'\(-5\).*object 0 \(id 1\).*2\^31'):
        gpu_handle.region_centers([line[:, :, :4635]], [1], (1, 1, 10))
    got_c, got_f = gpu_handle.region_centers([line[:, :, :46340]], [1])
    assert got_c.tolist() == [[0, 0, 46339]] and got_f.all()
    with pytest.raises(TypeError):
        gpu_handle.region_centers([crop.astype(np.int64)], [1])


def test_repeated_calls_agree_byte_for_byte(gpu_handle):
    rng = np.random.RandomState(12)
    crops = [rng.randint(0, 3, (9, 10, 11)).astype(np.uint64) for _ in range(20)]
    crops.append(np.where(rng.rand(11, 31, 33) < .95, 1, 0).astype(np.uint64))
    a = gpu_handle.region_centers(crops, [1] * len(crops), (2, 3, 5))
    b = gpu_handle.region_centers(crops, [1] * len(crops), (2, 3, 5))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[1].all()
