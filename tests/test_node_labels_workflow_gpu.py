"""NodeLabelWorkflow (target='local') end to end on the GPU on a small n5 volume: 24 x 48 x 80
fragments with maxId, blocks 10 x 32 x 32 (18 blocks, the last of every axis partial), 2 jobs.
Every block chunk equals the CPU restatement (tests/node_labels_ref.py) on that block, the merged
output equals the restatement's merge of the restated blocks -- the blocks the job skips by the
reference's rule (all-zero fragments; labels all ignore label) contribute nothing -- with the tie
rule (the smallest label) and the fill of nodes without a counted voxel."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import luigi_build

from cluster_tools_amd.utils import volume_utils as vu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.node_labels import serialization as S
import node_labels_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (24, 48, 80)
BLOCK_SHAPE = [10, 32, 32]
N_BLOCKS = 18
MAX_ID = 80
ZERO_BLOCK, IGNORED_BLOCK = 0, 10
TIED_NODE = 60


@pytest.fixture(scope='module')
def volume():
    """Fragments: cells of 6 x 12 x 16 voxels with the ids 1..80 (they cross the block borders at
    z = 10, 20 and y = 32), block 0 all zero (id 1 lies wholly in it: a node without any voxel).
    Labels: cells of 8 x 16 x 20 with the ids 1..36, block 10 all 0, and fragment 60 covered half
    by label 50 and half by label 40 (a tied maximum)."""
    z, y, x = np.meshgrid(np.arange(SHAPE[0]), np.arange(SHAPE[1]), np.arange(SHAPE[2]), indexing='ij')
    seg = (1 + (z // 6) * 20 + (y // 12) * 5 + x // 16).astype(np.uint64)
    seg[0:10, 0:32, 0:32] = 0
    gt = (1 + (z // 8) * 12 + (y // 16) * 4 + x // 20).astype(np.uint64)
    gt[10:20, 32:48, 32:64] = 0
    assert int(seg[12, 36, 64]) == TIED_NODE and (seg == TIED_NODE).sum() == 6 * 12 * 16
    gt[12:18, 36:48, 64:72] = 50
    gt[12:18, 36:48, 72:80] = 40
    assert seg.max() == MAX_ID and not (seg == 1).any()
    return seg, gt


def _run(tmp_path, seg, gt, **kwargs):
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    from cluster_tools_amd.node_labels import NodeLabelWorkflow
    cfg_dir = tmp_path / 'configs'
    cfg_dir.mkdir()
    g = BaseClusterTask.default_global_config()
    g['shebang'] = '#! ' + sys.executable
    g['block_shape'] = BLOCK_SHAPE
    (cfg_dir / 'global.config').write_text(json.dumps(g))
    path = str(tmp_path / 'data.n5')
    with vu.file_reader(path) as f:
        ds = f.create_dataset('seg', data=seg, chunks=(8, 16, 16))
        ds.attrs['maxId'] = MAX_ID
        f.create_dataset('gt', data=gt, chunks=tuple(min(c, s) for c, s in zip((8, 16, 16), gt.shape)))
    out_path, tmp_folder = str(tmp_path / 'out.n5'), str(tmp_path / 'tmp')
    task = NodeLabelWorkflow(tmp_folder=tmp_folder, config_dir=str(cfg_dir), target='local', max_jobs=2,
                             ws_path=path, ws_key='seg', input_path=path, input_key='gt', output_path=out_path,
                             output_key='node_labels', **kwargs)
    luigi_build(task, tmp_folder)
    return out_path, tmp_folder


def _check_blocks(out_path, tmp_folder, seg, labels_of, ignore_label, prefix=''):
    """Every block chunk against the restatement; -> the restated merge of the blocks."""
    blocking = Blocking([0, 0, 0], list(SHAPE), BLOCK_SHAPE)
    logs = ''.join(open(os.path.join(tmp_folder, 'logs', n)).read() for n in sorted(os.listdir(
        os.path.join(tmp_folder, 'logs'))) if n.startswith('block_node_labels_%s_' % prefix))
    restated, skipped = [], []
    with vu.file_reader(out_path, 'r') as f:
        ds = f['label_overlaps_%s' % prefix]
        assert tuple(ds.shape) == SHAPE and tuple(ds.chunks) == tuple(BLOCK_SHAPE) and str(ds.dtype) == 'uint64'
        assert ds.attrs['maxId'] == MAX_ID
        for block_id in range(N_BLOCKS):
            block = blocking.getBlock(block_id)
            bb = vu.block_to_bb(block)
            cid = tuple(b // s for b, s in zip(block.begin, BLOCK_SHAPE))
            ref = R.block_rows(seg[bb], labels_of(bb), ignore_label)
            assert 'processed block %i' % block_id in logs
            if ref is None:
                skipped.append(block_id)
                assert ds.read_chunk(cid) is None
                assert S.deserialize_overlap_chunk(ds.path, cid) == ({}, 0)
                continue
            restated.append(ref)
            np.testing.assert_array_equal(ds.read_chunk(cid), S.serialize_overlaps(ref))
            d, max_label = S.deserialize_overlap_chunk(ds.path, cid)
            assert d == R.rows_to_dict(ref) and max_label == int(ref[:, 1].max())
    return R.merge_rows(restated), skipped


@pytest.mark.parametrize('ignore_label', [None, 0])
def test_max_overlap(tmp_path, volume, ignore_label):
    seg, gt = volume
    out_path, tmp_folder = _run(tmp_path, seg, gt, ignore_label=ignore_label)
    merged, skipped = _check_blocks(out_path, tmp_folder, seg, lambda bb: gt[bb], ignore_label)
    assert skipped == ([ZERO_BLOCK] if ignore_label is None else [ZERO_BLOCK, IGNORED_BLOCK])
    # but for the skipped zero block (node 0 there) the merge is the whole volume's table
    whole = R.overlap_rows(seg, gt, ignore_label)
    zero = R.overlap_rows(seg[0:10, 0:32, 0:32], gt[0:10, 0:32, 0:32], ignore_label)
    np.testing.assert_array_equal(R.merge_rows([merged, zero]), whole)
    want = R.max_overlap(merged, MAX_ID + 1, ignore_label)
    with vu.file_reader(out_path, 'r') as f:
        ds = f['node_labels']
        assert tuple(ds.shape) == (MAX_ID + 1,) and tuple(ds.chunks) == (MAX_ID + 1,) and str(ds.dtype) == 'uint64'
        got = ds[:]
    np.testing.assert_array_equal(got, want)
    # the tie of fragment 60 (labels 40 and 50, 576 voxels each) goes to the smaller label
    d = R.rows_to_dict(merged)
    assert d[TIED_NODE] == {40: 576, 50: 576} and got[TIED_NODE] == 40
    # fragment 1 has no voxel: the fill
    assert 1 not in d and got[1] == 0
    assert os.path.exists(os.path.join(tmp_folder, 'merge_node_labels_max_ol_.log'))


@pytest.mark.parametrize('serialize_counts', [True, False])
def test_all_overlaps_with_prefix(tmp_path, volume, serialize_counts):
    seg, gt = volume
    out_path, tmp_folder = _run(tmp_path, seg, gt, ignore_label=0, max_overlap=False,
                                serialize_counts=serialize_counts, prefix='gt')
    merged, skipped = _check_blocks(out_path, tmp_folder, seg, lambda bb: gt[bb], 0, prefix='gt')
    assert skipped == [ZERO_BLOCK, IGNORED_BLOCK]
    want = merged.copy()
    if not serialize_counts:
        want[:, 2] = 0
    with vu.file_reader(out_path, 'r') as f:
        ds = f['node_labels']
        assert tuple(ds.shape) == (MAX_ID + 1,)
        np.testing.assert_array_equal(ds.read_chunk((0,)), S.serialize_overlaps(merged, serialize_counts))
        d, max_label = S.deserialize_overlap_chunk(ds.path, (0,))
    assert d == R.rows_to_dict(want) and max_label == 50
    for name in ('block_node_labels_gt.log', 'merge_node_labels_all_ol_gt.log',
                 'block_node_labels_job_gt_0.config', 'merge_node_labels_job_all_ol_gt_0.config',
                 os.path.join('logs', 'block_node_labels_gt_1.log'),
                 os.path.join('logs', 'merge_node_labels_all_ol_gt_0.log')):
        assert os.path.exists(os.path.join(tmp_folder, name)), name


def test_half_resolution_labels(tmp_path, volume):
    """A label volume of half the shape is read through vu.InterpolatedVolume(spline_order=0),
    block by block as the job does."""
    seg, gt = volume
    low = np.ascontiguousarray(gt[::2, ::2, ::2])
    out_path, tmp_folder = _run(tmp_path, seg, low, ignore_label=0)
    interp = vu.InterpolatedVolume(low, SHAPE, spline_order=0)
    merged, skipped = _check_blocks(out_path, tmp_folder, seg, lambda bb: interp[bb], 0)
    assert ZERO_BLOCK in skipped
    with vu.file_reader(out_path, 'r') as f:
        got = f['node_labels'][:]
    np.testing.assert_array_equal(got, R.max_overlap(merged, MAX_ID + 1, 0))
    assert len(np.unique(got)) > 10
