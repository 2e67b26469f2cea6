"""The numpy restatement of RegionCenters (tests/region_centers_ref.py) against scipy: the recorded
`np.argmax(distance_transform_edt(box, sampling=r))` of tests/golden/region_centers_scipy.npz
(scripts/make_region_centers_golden.py) and, where scipy is installed, live scipy on random boxes
with random integer samplings.  Exact: integer squared distances, first maximum in C order."""
import os

import numpy as np
import pytest

import region_centers_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'region_centers_scipy.npz')


def load_golden():
    """-> (kinds, boxes, resolutions (4, 3), argmax (n, 4))"""
    with np.load(GOLDEN) as z:
        shapes, argmax, res = z['shapes'], z['argmax'], z['resolutions']
        kinds = [str(k) for k in z['kinds']]
        flat = np.unpackbits(z['bits']).astype(bool)
    boxes, o = [], 0
    for s in shapes:
        n = int(np.prod(s))
        boxes.append(flat[o:o + n].reshape(tuple(int(v) for v in s)))
        o += n
    return kinds, boxes, res, argmax


def test_fixture_holds_the_cases():
    kinds, boxes, res, argmax = load_golden()
    assert len(boxes) >= 40 and argmax.shape == (len(boxes), 4)
    assert [tuple(r) for r in res] == [(1, 1, 1), (10, 1, 1), (1, 1, 10), (2, 3, 5)]
    for kind in ('random50', 'random80', 'random95', 'full', 'one_hole', 'shell', 'two_blobs', 'slab'):
        assert kind in kinds
    assert all(b.any() for b in boxes)
    # the rule of a box without background, on scipy's own outputs: the last voxel
    full = [(b, a) for k, b, a in zip(kinds, boxes, argmax) if k == 'full']
    assert len(full) >= 5
    for b, a in full:
        assert b.all() and (a == b.size - 1).all()
    # the slab's flat ties (the first maximum in C order moves with the resolution)
    slab = kinds.index('slab')
    got = [np.unravel_index(int(a), boxes[slab].shape) for a in argmax[slab][:3]]
    assert got == [(3, 3, 3), (1, 4, 4), (3, 3, 1)]


def test_restatement_equals_recorded_scipy():
    kinds, boxes, res, argmax = load_golden()
    for k, (box, want) in enumerate(zip(boxes, argmax)):
        for r, w in zip(res, want):
            c = R.box_center(box, tuple(int(v) for v in r))
            assert int(np.ravel_multi_index(c, box.shape)) == int(w), (k, kinds[k], box.shape, tuple(r))


def test_no_object_and_flat_tie():
    assert R.box_center(np.zeros((2, 3, 4), dtype=bool)) is None
    assert R.box_center(np.zeros((0, 3, 4), dtype=bool)) is None
    box = np.ones((1, 4, 4), dtype=bool)
    box[0, 0, 0] = False
    assert R.box_center(box) == (0, 3, 3)


def test_restatement_equals_live_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.RandomState(5)
    for k in range(300):
        shape = tuple(int(s) for s in rng.randint(1, 8, 3))
        box = rng.rand(*shape) < rng.choice([.5, .8, .95, 1.])
        if not box.any():
            continue
        r = tuple(int(v) for v in rng.randint(1, 12, 3))
        want = int(np.argmax(ndimage.distance_transform_edt(box, sampling=r)))
        got = int(np.ravel_multi_index(R.box_center(box, r), shape))
        assert got == want, (k, shape, r)
        if not box.all():
            d = ndimage.distance_transform_edt(box, sampling=r)
            np.testing.assert_array_equal(np.rint(d * d).astype(np.int64), R.squared_edt(box, r))
