"""Pass 2 of the two-pass watershed (`_ws_pass2`, two_pass_watershed.py:122-255) on the GPU
against the oracle, with the same initial seeds (pass-1 labels of the neighbours).

Bars: bit-exact against the oracle's flood model (the GPU's (C, d, label) order), and
VI <= 0.01 / adapted Rand <= 1e-3 against the vigra heap order (reference label 0 ignored
when a mask is used).
"""
import numpy as np
import pytest

from cluster_tools_amd.metrics import vi_scores, rand_scores
from oracle import oracle as O
from pass2_cases import (SCENARIOS, SPLIT_CASES, SF_SPARSE_MAX, SPLIT_ID_BASE, assert_split_preconditions, scenario, split_case, split_model,
                         whole_outer)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_pass2_matches_model_exactly(gpu_handle, name):
    config, block_shape, blocks = scenario(name)
    with O.flood_model():
        ref = O.ws_blocks(config, block_shape, blocks, pass_id=1)
    res = gpu_handle.ws_blocks(config, block_shape, blocks, pass_id=1)
    for r, g in zip(ref, res):
        assert g['status'] == r['status']
        np.testing.assert_array_equal(g['output'], r['output'])
        assert g['max_label'] == r['max_label']


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_pass2_fragments_vi(gpu_handle, name):
    config, block_shape, blocks = scenario(name)
    ref = O.ws_blocks(config, block_shape, blocks, pass_id=1)
    res = gpu_handle.ws_blocks(config, block_shape, blocks, pass_id=1)
    for b, r, g in zip(blocks, ref, res):
        assert g['status'] == r['status'] == 0
        ign = [0] if b.get('mask') is not None else None
        vis, vim = vi_scores(g['output'], r['output'], ign)
        are, _ = rand_scores(g['output'], r['output'], ign)
        print('%s block %d: VI %.2e, ARE %.2e' % (name, b['block_id'], vis + vim, are))
        assert vis + vim <= 0.01
        assert are <= 1e-3
        # the initial seeds survive as ids of the output (stitching across the checkerboard)
        init = b['initial_seeds']
        ib, ish = b['inner_begin'], g['output'].shape
        sl = tuple(slice(a, a + s) for a, s in zip(ib, ish))
        halo_ids = set(np.unique(init[init != 0] & np.uint64(0xFFFFFFFF)).tolist())
        assert halo_ids & set(np.unique(g['output']).tolist()) or not halo_ids
        assert g['output'].shape == init[sl].shape


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_pass2_whole_outer_matches_model(gpu_handle, name):
    """The inner block set to the outer block: what pass 2 computes in its halo (the size
    filter's removals there move the 2-D slice offsets and the regrow of the inner block)."""
    config, block_shape, blocks = scenario(name)
    blocks = [whole_outer(b) for b in blocks]
    with O.flood_model():
        ref = O.ws_blocks(config, block_shape, blocks, pass_id=1)
    res = gpu_handle.ws_blocks(config, block_shape, blocks, pass_id=1)
    for b, r, g in zip(blocks, ref, res):
        assert g['status'] == r['status']
        assert g['output'].shape == b['input'].shape
        np.testing.assert_array_equal(g['output'], r['output'])
        assert g['max_label'] == r['max_label']


@pytest.mark.parametrize('name', sorted(SPLIT_CASES))
def test_pass2_split_ids_match_model(gpu_handle, name):
    """Initial ids in several pieces, each id below the size filter and not excluded: the
    reference's apply_size_filter removes every piece (pass2_cases.py), whichever piece holds
    the id's first position."""
    assert_split_preconditions(name)
    config, block_shape, blocks, _ = split_case(name)
    res = gpu_handle.ws_blocks(config, block_shape, blocks, pass_id=1)
    t = gpu_handle.timings()
    for r, g in zip(split_model(name), res):
        assert g['status'] == r['status'] == 0
        np.testing.assert_array_equal(g['output'], r['output'])
        assert g['max_label'] == r['max_label']
    # the path under test: every block was planned sparse, and its walks met a label in pieces
    # (a size filter above kSfSparseMax: no walk at all)
    assert t['sf_sparse_blocks'] == 0, t
    assert t['sf_redo_blocks'] == (len(blocks) if config['size_filter'] <= SF_SPARSE_MAX else 0), t


def test_pass2_split_block_beside_a_walked_block(gpu_handle):
    """One batch, in both orders: a block whose walks meet split ids (handed back to the scan)
    and a block whose labels are all connected (walked), sharing the regrow bitmaps."""
    config, block_shape, (split,), _ = split_case('edges_3d')
    plain = whole_outer(scenario('3d', id_base=SPLIT_ID_BASE)[2][1])
    with O.flood_model():
        ref = [split_model('edges_3d')[0], O.ws_blocks(config, block_shape, [plain], pass_id=1)[0]]
    blocks = [split, plain]
    for order in ((0, 1), (1, 0)):
        res = gpu_handle.ws_blocks(config, block_shape, [blocks[i] for i in order], pass_id=1)
        t = gpu_handle.timings()
        assert (t['host_batches'], t['sf_sparse_blocks'], t['sf_redo_blocks']) == (1, 1, 1), t
        for i, g in zip(order, res):
            assert g['status'] == ref[i]['status'] == 0
            np.testing.assert_array_equal(g['output'], ref[i]['output'])
            assert g['max_label'] == ref[i]['max_label']


@pytest.mark.parametrize('name', sorted(SPLIT_CASES))
def test_pass2_split_ids_device_path(gpu_handle, name):
    import torch
    config, block_shape, blocks, _ = split_case(name)
    host = gpu_handle.ws_blocks(config, block_shape, blocks, pass_id=1)
    dev = []
    for b in blocks:
        d = dict(input=torch.from_numpy(b['input']).cuda(), block_id=b['block_id'], inner_begin=b['inner_begin'],
                 initial_seeds=torch.from_numpy(b['initial_seeds'].view(np.int64)).cuda(),
                 output=torch.zeros(tuple(b['inner_shape']), dtype=torch.int64, device='cuda'))
        if b.get('mask') is not None:
            d['mask'] = torch.from_numpy(np.ascontiguousarray(b['mask'], dtype=np.uint8)).cuda()
        dev.append(d)
    st = gpu_handle.ws_blocks_device(config, block_shape, dev, pass_id=1)
    for h, d, s in zip(host, dev, st):
        assert s[0] == h['status'] == 0
        assert s[1] == h['max_label']
        assert np.array_equal(d['output'].cpu().numpy().view(np.uint64), h['output'])


def test_pass2_empty_block_writes_nothing(gpu_handle):
    x = np.full((16, 40, 40), 0.7, np.float32)   # normalize -> all 0 < threshold: dt is None
    init = np.zeros(x.shape, np.uint64)
    init[:, :4] = 12345
    out = np.full((16, 32, 40), 9, np.uint64)
    b = dict(input=x, block_id=5, inner_begin=(0, 8, 0), inner_shape=(16, 32, 40), initial_seeds=init, out=out)
    res = gpu_handle.ws_blocks({}, (16, 32, 40), [b], pass_id=1)[0]
    assert res['status'] == 3
    assert (out == 9).all()


def test_pass2_device_path(gpu_handle):
    import torch
    config, block_shape, blocks = scenario('3d')
    host = gpu_handle.ws_blocks(config, block_shape, blocks, pass_id=1)
    dev = []
    for b in blocks:
        dev.append(dict(input=torch.from_numpy(b['input']).cuda(), block_id=b['block_id'],
                        inner_begin=b['inner_begin'],
                        initial_seeds=torch.from_numpy(b['initial_seeds'].view(np.int64)).cuda(),
                        output=torch.zeros(tuple(b['inner_shape']), dtype=torch.int64, device='cuda')))
    st = gpu_handle.ws_blocks_device(config, block_shape, dev, pass_id=1)
    for h, d, s in zip(host, dev, st):
        assert s[0] == 0
        assert np.array_equal(d['output'].cpu().numpy().view(np.uint64), h['output'])
