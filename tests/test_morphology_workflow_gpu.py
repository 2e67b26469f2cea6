"""MorphologyWorkflow (target='local') end to end on the GPU on a small n5 volume: 20 x 48 x 136
labels with maxId above the largest id present, blocks 8 x 16 x 64 (27 blocks, the last of every
axis partial), 2 block jobs and 2 merge jobs.  Every block chunk equals the CPU restatement
(tests/morphology_ref.py) on that block; the merged table equals the whole volume in exact
arithmetic: id, size, minima and maxima exactly, the centres within (k + 3) 2^-53 max(shape) of
S / n for an id held by k blocks (the roundings of the blocks' centres, of the k products, of the
k - 1 additions and of the division)."""
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import luigi_build

from cluster_tools_amd.utils import volume_utils as vu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.morphology import serialization as S
import morphology_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (20, 48, 136)
BLOCK_SHAPE = [8, 16, 64]
N_BLOCKS = 27
MAX_ID = 70      # ids 61..70 occur nowhere
SPRINKLED = 60
ZERO_BLOCK = 13  # block (1, 1, 1)


@pytest.fixture(scope='module')
def volume():
    """A coarse random grid of the ids 0..49 enlarged to cells of 5 x 12 x 34 voxels (they cross
    the block borders), single voxels of id 60 sprinkled in, and block 13 all zero."""
    rng = np.random.RandomState(11)
    coarse = rng.randint(0, 50, (4, 4, 4)).astype(np.uint64)
    coarse[0, 0, 0] = coarse[3, 3, 3] = 0  # id 0 also outside the zero block
    vol = np.ascontiguousarray(np.kron(coarse, np.ones((5, 12, 34), dtype=np.uint64)))
    assert vol.shape == SHAPE
    vol[rng.rand(*SHAPE) < .003] = SPRINKLED
    vol[8:16, 16:32, 64:128] = 0
    return vol


def _run(tmp_path, vol, prefix=''):
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    from cluster_tools_amd.morphology import MorphologyWorkflow
    cfg_dir = tmp_path / 'configs'
    cfg_dir.mkdir(exist_ok=True)
    g = BaseClusterTask.default_global_config()
    g['shebang'] = '#! ' + sys.executable
    g['block_shape'] = BLOCK_SHAPE
    (cfg_dir / 'global.config').write_text(json.dumps(g))
    path = str(tmp_path / 'data.n5')
    if not os.path.exists(path):
        with vu.file_reader(path) as f:
            ds = f.create_dataset('seg', data=vol, chunks=(8, 16, 32))
            ds.attrs['maxId'] = MAX_ID
    out_path, tmp_folder = str(tmp_path / 'out.n5'), str(tmp_path / ('tmp_' + prefix))
    task = MorphologyWorkflow(tmp_folder=tmp_folder, config_dir=str(cfg_dir), target='local', max_jobs=2,
                              max_jobs_merge=2, input_path=path, input_key='seg', output_path=out_path,
                              output_key='morphology' + prefix, prefix=prefix)
    luigi_build(task, tmp_folder)
    return out_path, tmp_folder


def _check_blocks(out_path, tmp_folder, vol, prefix):
    """Every block chunk against the restatement; -> how many blocks hold each id."""
    blocking = Blocking([0, 0, 0], list(SHAPE), BLOCK_SHAPE)
    assert blocking.numberOfBlocks == N_BLOCKS
    logs = ''.join(open(os.path.join(tmp_folder, 'logs', n)).read() for n in sorted(os.listdir(
        os.path.join(tmp_folder, 'logs'))) if n.startswith('block_morphology_%s_' % prefix))
    holders = {}
    with vu.file_reader(out_path, 'r') as f:
        ds = f['morphology_%s' % prefix]
        assert tuple(ds.shape) == SHAPE and tuple(ds.chunks) == tuple(BLOCK_SHAPE) and str(ds.dtype) == 'float64'
        for block_id in range(N_BLOCKS):
            block = blocking.getBlock(block_id)
            cid = tuple(b // s for b, s in zip(block.begin, BLOCK_SHAPE))
            assert 'processed block %i' % block_id in logs
            if block_id == ZERO_BLOCK:
                assert 'block %i is empty' % block_id in logs
                assert ds.read_chunk(cid) is None  # the all-zero block's chunk is absent
                continue
            ref = R.block_morphology(vol[vu.block_to_bb(block)], block.begin)
            np.testing.assert_array_equal(ds.read_chunk(cid), S.serialize_morphology(ref))
            for i in ref[:, 0]:
                holders[int(i)] = holders.get(int(i), 0) + 1
    assert logs.count(' is empty') == 1
    return holders


def _check_table(out_path, key, vol, holders):
    # the zero block is skipped by the reference's rule: its voxels are in no chunk
    exact = R.volume_exact(vol)
    zero_block = vol[8:16, 16:32, 64:128].size
    with vu.file_reader(out_path, 'r') as f:
        ds = f[key]
        assert tuple(ds.shape) == (MAX_ID + 1, 11) and tuple(ds.chunks) == (MAX_ID + 1, 11)
        assert str(ds.dtype) == 'float64'
        got = ds[:]
    assert holders[0] >= 2 and max(holders.values()) >= 8
    for i in range(MAX_ID + 1):
        if i not in exact:
            assert not got[i].any(), i  # an absent id: eleven zeros
            continue
        n, com, lo, hi = exact[i]
        if i == 0:
            # id 0 without the skipped block: compare with the volume in which that block is cut out
            rest = np.ones(SHAPE, dtype=bool)
            rest[8:16, 16:32, 64:128] = False
            zz, yy, xx = np.nonzero((vol == 0) & rest)
            n = len(zz)
            assert n == exact[0][0] - zero_block
            com = tuple(Fraction(int(c.sum()), n) for c in (zz, yy, xx))
            lo = tuple(int(c.min()) for c in (zz, yy, xx))
            hi = tuple(int(c.max()) for c in (zz, yy, xx))
        assert got[i, 0] == i and got[i, 1] == n
        assert tuple(got[i, 5:8]) == lo and tuple(got[i, 8:11]) == hi
        bound = Fraction(R.centre_bound(holders[i], SHAPE))
        for a in range(3):
            err = abs(Fraction(float(got[i, 2 + a])) - com[a])
            assert err <= bound, (i, a, float(err), float(bound))
    assert not got[61:].any() and got[SPRINKLED, 1] > 100


def test_morphology_workflow(tmp_path, volume):
    out_path, tmp_folder = _run(tmp_path, volume)
    holders = _check_blocks(out_path, tmp_folder, volume, '')
    _check_table(out_path, 'morphology', volume, holders)
    for name in ('block_morphology_.log', 'merge_morphology_.log', 'block_morphology_job__1.config',
                 'merge_morphology_job__1.config', os.path.join('logs', 'block_morphology__1.log'),
                 os.path.join('logs', 'merge_morphology__1.log')):
        assert os.path.exists(os.path.join(tmp_folder, name)), name
    # a second run with a prefix leaves a second temporary key beside the first
    out_path, tmp_folder = _run(tmp_path, volume, prefix='b')
    holders_b = _check_blocks(out_path, tmp_folder, volume, 'b')
    assert holders_b == holders
    _check_table(out_path, 'morphologyb', volume, holders)
    with vu.file_reader(out_path, 'r') as f:
        assert tuple(f['morphology_'].shape) == tuple(f['morphology_b'].shape) == SHAPE
        np.testing.assert_array_equal(f['morphology'][:], f['morphologyb'][:])
