"""The size filter's block entry points on the GPU (ctws_set_discard_u64, ctws_size_filter_blocks
and _device; k_sizefilter.hip and the uint64 / raw-height-map mode of k_seeded.hip) against the
CPU restatement of `apply_block` (tests/size_filter_ref.py; postprocess/background_size_filter.py:
110-130, filling_size_filter.py:112-136).

Bars: the background filter equals numpy exactly; the fill equals the oracle's flood model
bit-exactly on every height map, and against vigra's heap order it stays within VI <= 0.01 and
adapted Rand <= 1e-3 where the model itself equals the heap order (float32 smoothed map), while on
the tie-dominated maps (uint8, exact plateaus) its VI to the heap order must be the model's own
(to 1e-9; the gap is computed here, measured on the CPU: uint8 0.034, plateaus 0.029).

X = 72 is no multiple of the 64-lane wave, so id runs cross waves and rows."""
import numpy as np
import pytest

from cluster_tools_amd.metrics import vi_scores, rand_scores
from oracle import oracle as O
import size_filter_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (24, 80, 72)
BIG = np.uint64(2 ** 33)


class _Base:
    def __init__(self):
        from scipy.ndimage import gaussian_filter
        self.labels, self.raw = R.fragments(SHAPE)
        self.discard = R.ids_below_median(self.labels)
        self.f32 = gaussian_filter(self.raw, 1.0).astype(np.float32)
        self.hmaps = {'f32': self.f32, 'uint8': np.round(self.f32 * 255).astype(np.uint8), 'plateaus': self.raw,
                      # both bytes in use, a minimum above 0 (the fill floods the raw values, not normalized)
                      'uint16': (7 + np.round(65000 * self.f32)).astype(np.uint16)}
        self._ref = {}

    def ref(self, name):
        """(model, heap order) of the fill on height map `name`, computed once."""
        if name not in self._ref:
            with O.flood_model():
                _, model = R.apply_block(self.labels, self.discard, self.hmaps[name])
            _, heap = R.apply_block(self.labels, self.discard, self.hmaps[name])
            self._ref[name] = (model, heap)
        return self._ref[name]


@pytest.fixture(scope='module')
def base():
    b = _Base()
    assert len(np.unique(b.labels)) == 75 and len(b.discard) == 37  # the documented input
    return b


@pytest.mark.parametrize('name', ['f32', 'uint8', 'plateaus'])
def test_fill_equals_flood_model(gpu_handle, base, name):
    model, heap = base.ref(name)
    gpu_handle.set_discard_ids(base.discard)
    res = gpu_handle.size_filter_blocks([dict(labels=base.labels, hmap=base.hmaps[name])], fill=True)[0]
    assert res['status'] == R.WRITTEN, gpu_handle.last_error()
    vi = sum(vi_scores(res['output'], heap))
    are = rand_scores(res['output'], heap)[0]
    gap = sum(vi_scores(model, heap))
    print('%s: VI to heap order %.3e (model %.3e), ARE %.3e, exact-vs-model %s'
          % (name, vi, gap, are, np.array_equal(res['output'], model)))
    np.testing.assert_array_equal(res['output'], model)
    if name == 'f32':
        assert vi <= 0.01 and are <= 1e-3
    else:
        assert abs(vi - gap) <= 1e-9
    assert res['max_label'] == int(res['output'].max())
    assert not np.isin(res['output'], base.discard).any() and (res['output'] != 0).all()


def test_fill_uint16_height_map(gpu_handle, base):
    """A uint16 height map (k_sf_hmap's sf_cast<uint16_t>, the staging at element size 2): bit-exact
    against the model and, with 65,000 levels, within the bars against vigra's heap order too (the
    model's own VI to it, measured on the CPU: 5.1e-4).  The fill has no prep pass: prep_kernel -1."""
    model, heap = base.ref('uint16')
    hm = base.hmaps['uint16']
    assert hm.dtype == np.uint16 and hm.min() >= 7 and hm.max() > 256 and ((hm & 0xFF) != 0).any()
    gpu_handle.set_discard_ids(base.discard)
    res = gpu_handle.size_filter_blocks([dict(labels=base.labels, hmap=hm)], fill=True)[0]
    assert res['status'] == R.WRITTEN, gpu_handle.last_error()
    assert gpu_handle.timings()['prep_kernel'] == -1
    np.testing.assert_array_equal(res['output'], model)
    vi = sum(vi_scores(res['output'], heap))
    print('uint16: VI to heap order %.3e (model %.3e)' % (vi, sum(vi_scores(model, heap))))
    assert vi <= 0.01
    assert res['max_label'] == int(res['output'].max())
    assert not np.isin(res['output'], base.discard).any() and (res['output'] != 0).all()


def test_fill_keeps_64_bit_ids(gpu_handle, base):
    """Un-relabelled watershed ids pass 2^32: the f32 case with 2^33 added to every id."""
    model, _ = base.ref('f32')
    big = np.where(base.labels != 0, base.labels + BIG, np.uint64(0))
    gpu_handle.set_discard_ids(base.discard + BIG)
    res = gpu_handle.size_filter_blocks([dict(labels=big, hmap=base.f32)], fill=True)[0]
    assert res['status'] == R.WRITTEN, gpu_handle.last_error()
    np.testing.assert_array_equal(res['output'], np.where(model != 0, model + BIG, np.uint64(0)))
    assert res['max_label'] == int(model.max()) + 2 ** 33


def test_reserved_id_fails_its_block_only(gpu_handle, base):
    model, _ = base.ref('f32')
    bad = base.labels.copy()
    bad[3, 3, 3] = np.uint64(2 ** 64 - 1)
    out = np.full(SHAPE, 5, np.uint64)
    gpu_handle.set_discard_ids(base.discard)
    res = gpu_handle.size_filter_blocks([dict(labels=bad, hmap=base.f32, out=out),
                                         dict(labels=base.labels, hmap=base.f32)], fill=True)
    assert res[0]['status'] == R.FAILED and '2^64 - 1' in gpu_handle.last_error()
    assert (out == 5).all()
    assert res[1]['status'] == R.WRITTEN
    np.testing.assert_array_equal(res[1]['output'], model)


def test_f64_height_map_fails_with_reason(gpu_handle, base):
    gpu_handle.set_discard_ids(base.discard)
    res = gpu_handle.size_filter_blocks([dict(labels=base.labels, hmap=base.f32.astype(np.float64))], fill=True)[0]
    assert res['status'] == R.FAILED and 'float64' in gpu_handle.last_error()


def _membership_sets(base):
    ids = np.unique(base.labels)
    rng = np.random.default_rng(5)
    # 100,000 ids of which only the 37 occur in the block: once within a bitmap's range, once
    # spread over 2^40 so that the set stays a sorted table
    others = np.setdiff1d(np.arange(100, 400000, dtype=np.uint64), ids)
    dense = np.union1d(rng.choice(others, 100000 - len(base.discard), replace=False), base.discard)
    far = rng.integers(2 ** 20, 2 ** 40, size=100000 - len(base.discard), dtype=np.int64).astype(np.uint64)
    sparse = np.union1d(far, base.discard)
    return {'empty': np.zeros(0, np.uint64), 'one': base.discard[:1], 'all': ids,
            'dense_100k': dense, 'sparse_100k': sparse,
            'no_bitmap': np.union1d(ids[::2], np.array([1, 2 ** 40], np.uint64))}


@pytest.mark.parametrize('name', ['empty', 'one', 'all', 'dense_100k', 'sparse_100k', 'no_bitmap'])
def test_membership_background(gpu_handle, base, name):
    discard = _membership_sets(base)[name]
    gpu_handle.set_discard_ids(discard)
    res = gpu_handle.size_filter_blocks([dict(labels=base.labels)])[0]
    st, exp = R.apply_block(base.labels, discard)
    assert res['status'] == st == (R.COPIED if name == 'empty' else R.WRITTEN)
    np.testing.assert_array_equal(res['output'], exp)
    np.testing.assert_array_equal(exp, np.where(np.isin(base.labels, discard), np.uint64(0), base.labels))
    assert res['max_label'] == int(exp.max())


@pytest.mark.parametrize('big', [False, True])
def test_membership_run_shapes(gpu_handle, big):
    """One id throughout (a single run head per wave) and ids alternating along x (every lane a
    run head), kept and discarded, with ids in a bitmap's range and beyond it."""
    off = np.uint64(2 ** 40) if big else np.uint64(0)
    const = np.full(SHAPE, 7, np.uint64) + off
    alt = (np.indices(SHAPE).sum(0) % 2).astype(np.uint64) * np.uint64(2) + np.uint64(7) + off  # 7 / 9
    for discard in ([7], [9], [7, 9], [8]):
        discard = np.array([1] + discard, np.uint64) + off
        discard[0] = 1
        gpu_handle.set_discard_ids(discard)
        res = gpu_handle.size_filter_blocks([dict(labels=const), dict(labels=alt)])
        for r, lab in zip(res, (const, alt)):
            st, exp = R.apply_block(lab, discard)
            assert r['status'] == st
            if exp is not None:
                np.testing.assert_array_equal(r['output'], exp)


def test_statuses(gpu_handle, base):
    gpu_handle.set_discard_ids(base.discard)
    out = np.full(SHAPE, 5, np.uint64)
    kept = np.where(np.isin(base.labels, base.discard), np.uint64(0), base.labels)  # no discard id left
    for fill in (False, True):
        res = gpu_handle.size_filter_blocks([dict(labels=np.zeros(SHAPE, np.uint64), hmap=base.f32, out=out),
                                             dict(labels=kept, hmap=base.f32)], fill=fill)
        assert res[0]['status'] == R.ZERO and (out == 5).all()
        assert res[1]['status'] == R.COPIED
        np.testing.assert_array_equal(res[1]['output'], kept)


def test_every_id_discarded_is_auto_seeded(gpu_handle, base):
    """No seed left: vigra seeds from the strict minima of the height map (ids 1..n), a quirk of
    the reference that is kept."""
    discard = np.unique(base.labels)
    with O.flood_model():
        st, model = R.apply_block(base.labels, discard, base.f32)
    gpu_handle.set_discard_ids(discard)
    res = gpu_handle.size_filter_blocks([dict(labels=base.labels, hmap=base.f32)], fill=True)[0]
    assert res['status'] == st == R.WRITTEN
    np.testing.assert_array_equal(res['output'], model)
    assert res['max_label'] == int(model.max()) > 75


@pytest.fixture(scope='module')
def batch():
    from scipy.ndimage import gaussian_filter
    blocks = []
    for i, sh in enumerate([(16, 64, 64), (10, 50, 90), SHAPE]):
        lab, raw = R.fragments(sh, seed=20 + i)
        blocks.append(dict(labels=lab + np.uint64(1000 * i), hmap=gaussian_filter(raw, 1.0).astype(np.float32)))
    discard = np.unique(np.concatenate([R.ids_below_median(b['labels']) for b in blocks]))
    return blocks, discard


def test_batch_equals_single(gpu_handle, batch):
    blocks, discard = batch
    gpu_handle.set_discard_ids(discard)
    for fill in (False, True):
        together = gpu_handle.size_filter_blocks(blocks, fill=fill)
        for b, t in zip(blocks, together):
            single = gpu_handle.size_filter_blocks([b], fill=fill)[0]
            assert single['status'] == t['status'] == R.WRITTEN
            np.testing.assert_array_equal(single['output'], t['output'])


def test_device_tensors_equal_host_path(gpu_handle, batch):
    import torch
    blocks, discard = batch
    gpu_handle.set_discard_ids(discard)
    dev = [dict(labels=torch.from_numpy(b['labels'].view(np.int64)).to('cuda:0'),
                hmap=torch.from_numpy(b['hmap']).to('cuda:0')) for b in blocks]
    dev.append(dict(labels=torch.zeros(SHAPE, dtype=torch.int64, device='cuda:0'),
                    hmap=torch.zeros(SHAPE, dtype=torch.float32, device='cuda:0'),
                    out=torch.full(SHAPE, 5, dtype=torch.int64, device='cuda:0')))
    for fill in (False, True):
        host = gpu_handle.size_filter_blocks(blocks, fill=fill)
        res = gpu_handle.size_filter_blocks_device(dev, fill=fill)
        for hr, dr in zip(host, res):
            assert hr['status'] == dr['status'] and hr['max_label'] == dr['max_label']
            np.testing.assert_array_equal(dr['output'].cpu().numpy().view(np.uint64), hr['output'])
        assert res[3]['status'] == R.ZERO and bool((res[3]['output'] == 5).all())
    # in place: the output is the labels' own tensor
    lab = dev[2]['labels'].clone()
    res = gpu_handle.size_filter_blocks_device([dict(labels=lab, hmap=dev[2]['hmap'], out=lab)], fill=True)[0]
    np.testing.assert_array_equal(lab.cpu().numpy().view(np.uint64), host[2]['output'])


def test_replaced_discard_set_takes_effect(gpu_handle, base):
    for discard in (base.discard, base.discard[:5], np.zeros(0, np.uint64), base.discard[5:]):
        gpu_handle.set_discard_ids(discard)
        res = gpu_handle.size_filter_blocks([dict(labels=base.labels)])[0]
        st, exp = R.apply_block(base.labels, discard)
        assert res['status'] == st
        np.testing.assert_array_equal(res['output'], exp)
    with pytest.raises(Exception):
        gpu_handle.set_discard_ids(np.array([5, 3], np.uint64))  # not ascending
