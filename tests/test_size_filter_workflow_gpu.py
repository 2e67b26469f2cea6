"""SizeFilterWorkflow (target='local') end to end on the GPU, on a small n5 volume: the background
and the filling variant, with and without the relabel, in place and to another dataset, against
the CPU restatement of `apply_block` (tests/size_filter_ref.py) applied block by block with the
GLOBAL voxel counts.  The labels are put together so that one block is all 0, one holds only
large ids, and one fragment straddles a block face with each half below the threshold and their
sum above it: it must survive, which is the point of counting over the whole volume."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import luigi_build

from cluster_tools_amd.utils import volume_utils as vu
from cluster_tools_amd.utils.blocking import Blocking
from oracle import oracle as O
import size_filter_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (32, 96, 96)
BLOCK_SHAPE = [16, 48, 48]
THRESHOLD = 200
STRADDLER = np.uint64(999999)


class _Volume:
    def __init__(self):
        from scipy.ndimage import gaussian_filter
        from cluster_tools_amd.synthetic import boundary_map
        self.blocking = Blocking([0, 0, 0], list(SHAPE), BLOCK_SHAPE)
        bvol = int(np.prod(BLOCK_SHAPE))
        labels = np.zeros(SHAPE, np.uint64)
        for bid in range(self.blocking.numberOfBlocks):
            bb = vu.block_to_bb(self.blocking.getBlock(bid))
            if bid == 0:
                continue  # all 0
            if bid == 1:  # two large ids only
                labels[bb] = np.uint64(bid * bvol + 1)
                labels[bb][:, :24] = np.uint64(bid * bvol + 2)
                continue
            frag, _ = R.fragments(tuple(BLOCK_SHAPE), seed=30 + bid)
            labels[bb] = frag + np.uint64(bid * bvol)  # un-relabelled watershed ids
        # blocks 2 and 3 share the face x = 48: 4 x 6 x 5 = 120 voxels on either side
        labels[2:6, 50:56, 43:53] = STRADDLER
        self.labels = labels
        self.hmap = gaussian_filter(boundary_map(SHAPE, seed=4), 1.0).astype(np.float32)
        ids, counts = np.unique(labels, return_counts=True)
        self.discard = ids[counts < THRESHOLD].astype(np.uint64)
        assert 0 < len(self.discard) < len(ids) - 1
        for bid in (2, 3):  # each half is below the threshold, the fragment is not
            half = (labels[vu.block_to_bb(self.blocking.getBlock(bid))] == STRADDLER).sum()
            assert 0 < half < THRESHOLD
        assert STRADDLER not in self.discard
        self._expected = {}

    def expected(self, fill):
        """(filtered volume on a zero background, statuses per block)"""
        if fill not in self._expected:
            out = np.zeros(SHAPE, np.uint64)
            statuses = []
            for bid in range(self.blocking.numberOfBlocks):
                bb = vu.block_to_bb(self.blocking.getBlock(bid))
                with O.flood_model():
                    st, res = R.apply_block(self.labels[bb], self.discard, self.hmap[bb] if fill else None)
                statuses.append(st)
                if res is not None:
                    out[bb] = res
            assert statuses[0] == R.ZERO and statuses[1] == R.COPIED and R.WRITTEN in statuses
            self._expected[fill] = out
        return self._expected[fill]


@pytest.fixture(scope='module')
def volume():
    return _Volume()


def _setup(tmp_path, volume, fill, in_place):
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    cfg_dir = tmp_path / 'configs'
    cfg_dir.mkdir()
    g = BaseClusterTask.default_global_config()
    g['shebang'] = '#! ' + sys.executable
    g['block_shape'] = BLOCK_SHAPE
    (cfg_dir / 'global.config').write_text(json.dumps(g))
    path = str(tmp_path / 'data.n5')
    chunks = tuple(b // 2 for b in BLOCK_SHAPE)
    with vu.file_reader(path) as f:
        ds = f.create_dataset('labels', data=volume.labels, chunks=chunks)
        ds.attrs['maxId'] = int(volume.labels.max())
        # in place the height map is 4-D: the filter takes its channel 0
        if fill and in_place:
            f.create_dataset('hmap', data=np.stack([volume.hmap, 1 - volume.hmap]), chunks=(1,) + chunks)
        elif fill:
            f.create_dataset('hmap', data=volume.hmap, chunks=chunks)
    return str(cfg_dir), path


@pytest.mark.parametrize('fill', [False, True])
@pytest.mark.parametrize('relabel', [True, False])
@pytest.mark.parametrize('in_place', [True, False])
def test_size_filter_workflow(tmp_path, volume, fill, relabel, in_place):
    from cluster_tools_amd.postprocess import SizeFilterWorkflow
    cfg_dir, path = _setup(tmp_path, volume, fill, in_place)
    tmp_folder = str(tmp_path / 'tmp')
    out_path = path if in_place else str(tmp_path / 'out.n5')
    out_key = 'labels' if in_place else 'filtered'
    hmap_kw = dict(hmap_path=path, hmap_key='hmap') if fill else {}
    task = SizeFilterWorkflow(tmp_folder=tmp_folder, config_dir=cfg_dir, max_jobs=2, target='local',
                              input_path=path, input_key='labels', output_path=out_path, output_key=out_key,
                              size_threshold=THRESHOLD, relabel=relabel, **hmap_kw)
    luigi_build(task, tmp_folder)

    np.testing.assert_array_equal(np.load(os.path.join(tmp_folder, 'discard_ids.npy')), volume.discard)
    exp = volume.expected(fill)
    with vu.file_reader(out_path, 'r') as f:
        res = f[out_key][:]
        max_id = f[out_key].attrs.get('maxId', None)
        table = f['relabel_size_filter'][:] if relabel else None
        assert relabel or 'relabel_size_filter' not in f
    # the straddling fragment survives with all its voxels
    assert ((exp == STRADDLER) == (volume.labels == STRADDLER)).all()
    if not relabel:
        np.testing.assert_array_equal(res, exp)
        assert max_id == int(volume.labels.max())
        return
    ids = np.unique(exp)
    assert ids[0] == 0
    np.testing.assert_array_equal(table[:, 0], ids)
    np.testing.assert_array_equal(table[:, 1], np.arange(len(ids), dtype=np.uint64))  # 0 kept, then 1..n
    np.testing.assert_array_equal(res, np.searchsorted(ids, exp).astype(np.uint64))
    np.testing.assert_array_equal(np.unique(res), np.arange(len(ids), dtype=np.uint64))
    assert max_id == len(ids) - 1
