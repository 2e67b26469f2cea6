"""Two-pass (checkerboard) scenarios for the pass-2 parity tests.

A small volume is cut into a 2 x 2 (y, x) block grid with a halo; the checkerboard colour of
block 0 (blocks 0 and 3) runs pass 1 (`_ws_block`) in the oracle and writes a full output
volume, then the other colour (blocks 1 and 2) runs `_ws_pass2` with
`initial_seeds = out[outer bb]` (two_pass_watershed.py:224-228).  Both the GPU and the oracle
pass 2 see the same initial seeds, so pass 2 is compared on its own.
"""
import numpy as np

from cluster_tools_amd.synthetic import boundary_map, ellipsoid_mask
from oracle import oracle as O

VOL = (24, 128, 128)
GRID_BLOCK = (24, 64, 64)

D3 = dict(apply_dt_2d=False, apply_ws_2d=False)

# name -> (task config, halo, block-id base, masked[, block-id stride])
# '2d_collide': block ids 2^17 apart, so every block_id * prod(block_shape) (V = 3 * 2^15) is
# 0 mod 2^32 -- the modular coincidence of a z-halo grid with V = 2^22 and gy * gx = 1024: the
# pass-2 block's new seeds (uint32 offset + local id) take the same uint32 values as the
# neighbours' pass-1 ids in its halo, and relabelConsecutive merges them
# (two_pass_watershed.py:147-155)
SCENARIOS = {
    '3d': (dict(D3), (0, 16, 16), 0, False),
    '2d': ({}, (0, 16, 16), 0, False),
    '3d_mask': (dict(D3), (0, 16, 16), 0, True),
    '2d_mask': ({}, (0, 16, 16), 0, True),
    '3d_wrap': (dict(D3), (0, 16, 16), 44000, False),     # block_id * V >= 2^32 (Appendix B.2)
    '2d_wrap': ({}, (0, 12, 20), 44000, False),
    '3d_nofilter': (dict(D3, size_filter=0), (0, 16, 16), 0, False),
    '3d_bigfilter': (dict(D3, size_filter=400), (0, 16, 16), 0, False),
    '2d_dt3d': (dict(apply_dt_2d=False), (0, 16, 16), 0, False),
    '2d_collide': ({}, (0, 16, 16), 0, False, 1 << 17),
    '2d_collide_mask': ({}, (0, 16, 16), 0, True, 1 << 17),
}


def _blocks(block_shape, halo):
    gy, gx = VOL[1] // GRID_BLOCK[1], VOL[2] // GRID_BLOCK[2]
    out = []
    for by in range(gy):
        for bx in range(gx):
            beg = (0, by * GRID_BLOCK[1], bx * GRID_BLOCK[2])
            end = tuple(b + s for b, s in zip(beg, GRID_BLOCK))
            obeg = tuple(max(0, b - h) for b, h in zip(beg, halo))
            oend = tuple(min(v, e + h) for v, e, h in zip(VOL, end, halo))
            out.append(dict(local_id=by * gx + bx, colour=(by + bx) % 2,
                            outer=tuple(slice(a, b) for a, b in zip(obeg, oend)),
                            inner_begin=tuple(b - o for b, o in zip(beg, obeg)),
                            inner=tuple(slice(a, b) for a, b in zip(beg, end))))
    return out


def scenario(name, seed=3, id_base=None):
    """-> (config, block_shape, list of pass-2 block dicts with initial_seeds).
    id_base overrides the scenario's block-id base."""
    config, halo, base, masked = SCENARIOS[name][:4]
    id_base = base if id_base is None else id_base
    stride = SCENARIOS[name][4] if len(SCENARIOS[name]) > 4 else 1
    config = dict(config, halo=list(halo))
    x = boundary_map(VOL, seed=seed)
    mask = ellipsoid_mask(VOL) if masked else None
    # the ids are block_id * prod(block_shape): the task's block_shape is the grid block
    block_shape = GRID_BLOCK
    out = np.zeros(VOL, np.uint64)
    blocks = _blocks(block_shape, halo)

    def as_block(b):
        d = dict(input=x[b['outer']], block_id=id_base + b['local_id'] * stride, inner_begin=b['inner_begin'],
                 inner_shape=GRID_BLOCK, crop_relabel=sum(halo) > 0)
        if mask is not None:
            d['mask'] = mask[b['outer']]
        return d

    first = [b for b in blocks if b['colour'] == 0]
    res = O.ws_blocks(config, block_shape, [as_block(b) for b in first])
    for b, r in zip(first, res):
        if r['status'] in (0, 2):
            out[b['inner']] = r['output']
    second = []
    for b in blocks:
        if b['colour'] != 1:
            continue
        d = as_block(b)
        d['crop_relabel'] = False
        d['initial_seeds'] = out[b['outer']].copy()
        second.append(d)
    return config, block_shape, second


# ---- whole-outer observation and planted split ids --------------------------------------------
# Pass 2 writes only the inner block, so what its size filter does in the halo is invisible to a
# comparison of the written output.  whole_outer() makes the inner block the outer block: the
# ABI accepts it, and the whole uint64 result of `_apply_watershed_with_seeds` is compared.
#
# In pass 2 a label is "every voxel that carried one initial id", which need not be connected (a
# pass-1 segment clipped by the outer block, or cut by a 2-D slice).  The generators below plant
# such ids on purpose: fresh initial ids PLANT_ID0 + k (below 2^32, colliding with nothing) in
# several small pieces, in blocks whose ids start at SPLIT_ID_BASE * prod(block_shape), so that
# no relabelled id equals an initial id and `exclude=` (two_pass_watershed.py:160,201) keeps
# none of them: the reference's apply_size_filter removes every piece of a small one.
PLANT_ID0 = 3_000_000_000
SPLIT_ID_BASE = 1000
SF_SPARSE_MAX = 64     # kSfSparseMax (k_post.hip): the largest size filter the sparse walk takes


def whole_outer(block):
    """The pass-2 block with its inner block set to the whole outer block."""
    d = dict(block, inner_begin=(0, 0, 0), inner_shape=tuple(block['input'].shape[-3:]))
    d.pop('out', None)
    return d


def _free_spot(rng, seeded, near, h, w):
    """A random top-left corner of an h x w patch on seeded voxels, none of them within 3 voxels
    of an earlier patch (near); None if there is no such place."""
    H, W = seeded.shape
    ok = np.ones((H - h + 1, W - w + 1), bool)
    for dy in range(h):
        for dx in range(w):
            ok &= seeded[dy:dy + H - h + 1, dx:dx + W - w + 1] & ~near[dy:dy + H - h + 1, dx:dx + W - w + 1]
    cand = np.argwhere(ok)
    if not len(cand):
        return None
    y, x = cand[rng.randint(len(cand))]
    near[max(0, y - 3):y + h + 3, max(0, x - 3):x + w + 3] = True
    return int(y), int(x)


def plant_split_ids(blocks, ws_2d, seed=1, per_plane=4, planes_3d=(4, 12, 20)):
    """Rewrite initial_seeds: in every slice (2-D ws) / in the z planes planes_3d (3-D), up to
    per_plane fresh ids of two 2 x 2 patches each, on voxels that carry an initial id, no patch
    within 3 voxels of another.  -> (blocks, per block the list of planted ids).
    A patch next to the unseeded part grows in the first flood, now and then to size_filter
    voxels or more: with the default seed none does, in any scenario of SPLIT_CASES
    (assert_split_preconditions, from the oracle alone)."""
    rng = np.random.RandomState(seed)
    out, planted = [], []
    k = 0
    for b in blocks:
        seeded = b['initial_seeds'] != 0
        init = b['initial_seeds'].copy()
        ids = []
        for z in (range(init.shape[0]) if ws_2d else planes_3d):
            near = np.zeros(init.shape[1:], bool)
            for _ in range(per_plane):
                spots = [_free_spot(rng, seeded[z], near, 2, 2) for _ in range(2)]
                if None in spots:
                    break
                for y, x in spots:
                    init[z, y:y + 2, x:x + 2] = PLANT_ID0 + k
                ids.append(PLANT_ID0 + k)
                k += 1
        out.append(dict(b, initial_seeds=init))
        planted.append(ids)
    return out, planted


def plant_boxes(block, ids_boxes):
    """Rewrite initial_seeds of one block: id k covers the boxes ids_boxes[k], each
    (z, y, x, h, w), all on voxels that carry an initial id.  -> (block, planted ids)."""
    init = block['initial_seeds'].copy()
    ids = []
    for k, boxes in enumerate(ids_boxes):
        for z, y, x, h, w in boxes:
            assert (block['initial_seeds'][z, y:y + h, x:x + w] != 0).all(), (k, z, y, x)
            assert (init[z, y:y + h, x:x + w] < PLANT_ID0).all(), (k, z, y, x)
            init[z, y:y + h, x:x + w] = PLANT_ID0 + k
        ids.append(PLANT_ID0 + k)
    return dict(block, initial_seeds=init), ids


# The edge ids, in the pass-2 block with local id 1 (outer 24 x 80 x 80 at (0, 0, 48); initial
# ids on x < 16 for y < 64 and on y >= 64 for x >= 16; the pieces of an id share a slice, as a
# 2-D label does).  One id each:
EDGE_BOXES = [
    # three pieces
    [(5, 10, 4, 2, 2), (5, 30, 8, 2, 2), (5, 50, 3, 2, 2)],
    # a single voxel at voxel index 0 of the outer block, the partner far away
    [(0, 0, 0, 1, 1), (0, 72, 60, 2, 2)],
    # a single voxel at the last voxel
    [(23, 79, 79, 1, 1), (23, 20, 5, 2, 2)],
    # a patch over x = 63 / 64: the bitmap word boundary of the 80-voxel rows
    [(10, 70, 63, 2, 2), (10, 30, 5, 2, 2)],
    # a patch on the seeded side of the inner face (x = 15 | 16): it grows into the unseeded part
    [(15, 40, 14, 2, 2), (15, 72, 40, 2, 2)],
]
# two pieces of 30 + 32 = 62 voxels: below size_filter 64 (the walk's queue length) and 65 (scan)
BIG_BOXES = [[(12, 5, 4, 5, 6), (12, 70, 30, 4, 8)]]

# name -> (scenario, planting, size_filter)
SPLIT_CASES = {
    'split_2d': ('2d', 'basic', 25),
    'split_3d': ('3d', 'basic', 25),
    'split_2d_mask': ('2d_mask', 'basic', 25),
    'split_3d_mask': ('3d_mask', 'basic', 25),
    'split_2d_wrap': ('2d_wrap', 'basic', 25),    # (keeps its own block-id base, above 1000)
    'edges_2d': ('2d', 'edges', 25),
    'edges_3d': ('3d', 'edges', 25),
    'big64_3d': ('3d', 'big', SF_SPARSE_MAX),
    'big65_3d': ('3d', 'big', SF_SPARSE_MAX + 1),
}
_SPLIT = {}


def split_case(name):
    """-> (config, block_shape, whole-outer pass-2 blocks with planted ids, per block the ids).
    Built once per name; the callers leave it unchanged."""
    if name not in _SPLIT:
        scen, planting, size_filter = SPLIT_CASES[name]
        config, block_shape, blocks = scenario(scen, id_base=max(SPLIT_ID_BASE, SCENARIOS[scen][2]))
        config = dict(config, size_filter=size_filter)
        if planting == 'basic':
            blocks, planted = plant_split_ids(blocks, config.get('apply_ws_2d', True))
        else:
            b, ids = plant_boxes(blocks[0], EDGE_BOXES if planting == 'edges' else BIG_BOXES)
            blocks, planted = [b], [ids]
        _SPLIT[name] = (config, block_shape, [whole_outer(b) for b in blocks], planted)
    return _SPLIT[name]


_MODEL = {}


def split_model(name, size_filter=None):
    """The flood model's whole-outer results of a split case (size_filter: override), once."""
    if (name, size_filter) not in _MODEL:
        config, block_shape, blocks, _ = split_case(name)
        if size_filter is not None:
            config = dict(config, size_filter=size_filter)
        with O.flood_model():
            _MODEL[name, size_filter] = O.ws_blocks(config, block_shape, blocks, pass_id=1)
    return _MODEL[name, size_filter]


def split_figures(name):
    """What makes a split case take the path under test, from the oracle alone; per block a dict:
    min_components / max_voxels of the planted ids in the unfiltered output (per slice in 2-D),
    planted / absent (planted ids missing in the filtered output), stale (voxels a walk of the
    first piece alone would leave behind), and k_sf_plan's conditions on the unfiltered output:
    nsmall, cap (N / 8 / size_filter), bare (slices / blocks without a label of size_filter
    voxels), zeros (unlabelled voxels), min_id and n_ids (min_id > n_ids: no relabelled id
    equals an initial id, so `exclude` keeps nothing)."""
    from scipy.ndimage import label
    config, _, blocks, planted = split_case(name)
    sf = config['size_filter']
    ws_2d = config.get('apply_ws_2d', True)
    figs = []
    for b, raw, ref, ids in zip(blocks, split_model(name, 0), split_model(name), planted):
        assert raw['status'] == ref['status'] == 0
        raw, ref = raw['output'], ref['output']
        planes = [raw[z] for z in range(raw.shape[0])] if ws_2d else [raw]
        f = dict(planted=len(ids), min_components=10 ** 9, max_voxels=0, absent=0, stale=0,
                 nsmall=0, bare=0, cap=raw.size // 8 // sf, zeros=int((raw == 0).sum()),
                 min_id=int(raw[raw != 0].min()), n_ids=0)
        present = set(np.unique(ref).tolist())
        for i in ids:
            f['absent'] += i not in present
            for p in planes:
                m = p == i
                if not m.any():
                    continue
                comp, n = label(m)
                f['min_components'] = min(f['min_components'], n)
                f['max_voxels'] = max(f['max_voxels'], int(m.sum()))
                if i not in present:
                    f['stale'] += int((m & (comp != comp.ravel()[np.flatnonzero(m)[0]])).sum())
            assert (raw == i).any(), 'planted id %d missing in the unfiltered output' % i
        for p in planes:
            u, c = np.unique(p[p != 0], return_counts=True)
            f['nsmall'] += int((c < sf).sum())
            f['bare'] += int(not (c >= sf).any())
            f['n_ids'] = max(f['n_ids'], len(u)) if ws_2d else len(u)
        figs.append(f)
    return figs


def assert_split_preconditions(name):
    """The case takes the sparse walk (size filter up to SF_SPARSE_MAX) with split small ids that
    the reference removes; beyond SF_SPARSE_MAX only the ids' shape is asserted (the scan)."""
    config, _, blocks, _ = split_case(name)
    sf = config['size_filter']
    for b, f in zip(blocks, split_figures(name)):
        print('%s block %d: %s' % (name, b['block_id'], f))
        assert f['planted'] > 0
        assert f['min_components'] >= 2, f
        assert f['max_voxels'] < sf, f
        assert f['absent'] * 10 >= f['planted'] * 9, f
        assert f['min_id'] > f['n_ids'], f
        if sf > SF_SPARSE_MAX:
            continue
        assert f['nsmall'] <= f['cap'], f
        assert f['bare'] == 0, f
        if b.get('mask') is None:
            assert f['zeros'] == 0, f
