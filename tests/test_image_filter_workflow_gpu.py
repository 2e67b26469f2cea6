"""ImageFilterLocal end to end on the GPU on a 20 x 48 x 80 n5 volume with blocks of (10, 24, 40):
float32 and uint8 inputs, halo [4, 8, 8] and no halo, the three filters at sigma 1.6 (radii 5 and 6:
both halos are below a radius on some axis, so the job warns), and a global roi.

The written dataset equals the restatement (tests/image_filter_ref.py, fed with the library's taps)
applied block by block with the same blocking, bit for bit.  It does not equal the filter of the
whole volume: the reference normalizes every outer block on its own (image_filter.py:110), and a
halo below the radius reflects at the block's faces; the test asserts that difference too."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import luigi_build

from cluster_tools_amd import ctws
from cluster_tools_amd.utils import volume_utils as vu
import image_filter_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (20, 48, 80)
BLOCK_SHAPE = [10, 24, 40]
SIGMA = 1.6


@pytest.fixture(scope='module')
def volumes():
    rng = np.random.RandomState(21)
    z, y, x = np.meshgrid(*[np.arange(n, dtype='float32') for n in SHAPE], indexing='ij')
    f = (np.sin(x / 7.0) + np.cos(y / 5.0) * 0.5 + z / 20.0 + rng.rand(*SHAPE) * 0.3).astype('float32')
    u = np.clip((f - f.min()) / (f.max() - f.min()) * 255, 0, 255).astype('uint8')
    return {'float32': f, 'uint8': u}


def _run(tmp_path, vol, name, filter_name, halo, roi=None):
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    from cluster_tools_amd.features import ImageFilterLocal
    cfg_dir = tmp_path / ('configs_' + name)
    cfg_dir.mkdir()
    g = BaseClusterTask.default_global_config()
    g['shebang'] = '#! ' + sys.executable
    g['block_shape'] = BLOCK_SHAPE
    if roi is not None:
        g['roi_begin'], g['roi_end'] = roi
    (cfg_dir / 'global.config').write_text(json.dumps(g))
    path = str(tmp_path / 'data.n5')
    with vu.file_reader(path) as f:
        if 'raw' not in f:
            f.create_dataset('raw', data=vol, chunks=(10, 24, 40))
    out_path, tmp_folder = str(tmp_path / 'out.n5'), str(tmp_path / ('tmp_' + name))
    task = ImageFilterLocal(tmp_folder=tmp_folder, config_dir=str(cfg_dir), max_jobs=2, input_path=path,
                            input_key='raw', output_path=out_path, output_key=name, filter_name=filter_name,
                            sigma=SIGMA, halo=halo)
    luigi_build(task, tmp_folder)
    with vu.file_reader(out_path, 'r') as f:
        ds = f[name]
        assert str(ds.dtype) == 'float32' and tuple(ds.shape) == SHAPE and tuple(ds.chunks) == (5, 12, 20)
        got = ds[:]
    logs = [open(os.path.join(tmp_folder, 'logs', 'image_filter_%i.log' % j)).read() for j in range(2)]
    return got, logs


CASES = [('gaussianSmoothing', 'float32', [4, 8, 8]), ('gaussianSmoothing', 'uint8', [0, 0, 0]),
         ('gaussianGradientMagnitude', 'uint8', [4, 8, 8]), ('gaussianGradientMagnitude', 'float32', [0, 0, 0]),
         ('laplacianOfGaussian', 'float32', [4, 8, 8]), ('laplacianOfGaussian', 'uint8', [0, 0, 0])]


@pytest.mark.parametrize('filter_name,dtype,halo', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_image_filter_workflow(tmp_path, volumes, filter_name, dtype, halo):
    vol = volumes[dtype]
    got, logs = _run(tmp_path, vol, 'resp', filter_name, halo)
    want = R.filter_blockwise(vol, BLOCK_SHAPE, halo, filter_name, SIGMA, taps_fn=ctws.filter_taps)
    np.testing.assert_array_equal(got, want)
    # per-block normalization and the reflected block faces: not the filter of the whole volume
    assert not np.array_equal(got, R.apply_filter(vol, filter_name, SIGMA, taps_fn=ctws.filter_taps))
    for log in logs:  # z: halo 4 (or 0) < radius 5 (or 6): every job says so once
        assert log.count('WARNING: the halo') == 1
        assert 'processed job' in log


def test_image_filter_workflow_roi(tmp_path, volumes):
    vol = volumes['float32']
    got, _ = _run(tmp_path, vol, 'roi', 'gaussianSmoothing', [4, 8, 8], roi=([0, 24, 0], [10, 48, 80]))
    want = R.filter_blockwise(vol, BLOCK_SHAPE, [4, 8, 8], 'gaussianSmoothing', SIGMA, block_ids=[2, 3],
                              taps_fn=ctws.filter_taps)
    np.testing.assert_array_equal(got, want)
    assert got[:10, 24:, :].any() and not got[10:].any() and not got[:, :24].any()  # the other blocks stay unwritten


def test_short_outer_block_fails_with_the_block_id():
    """Blocks of 4 slices without a halo cannot hold the radius 5 of sigma 1.6: the job fails on its
    first block and names it (datasets stood in by arrays: the loop is the job's)."""
    from cluster_tools_amd.features import image_filter as imf
    from cluster_tools_amd.utils.blocking import Blocking
    vol = np.random.RandomState(22).rand(8, 16, 16).astype('float32')
    out = np.zeros(vol.shape, 'float32')
    blocking = Blocking([0, 0, 0], list(vol.shape), [4, 16, 16])
    with pytest.raises(RuntimeError, match=r'block 1 \(outer shape \(4, 16, 16\)\).*axis z holds 4 voxels'):
        imf.run_filter_blocks(blocking, [1, 0], vol, out, [0, 0, 0], 'gaussianSmoothing', SIGMA, False)
    assert not out.any()
    imf.run_filter_blocks(blocking, [1, 0], vol, out, [2, 0, 0], 'gaussianSmoothing', SIGMA, False)
    np.testing.assert_array_equal(out, R.filter_blockwise(vol, [4, 16, 16], [2, 0, 0], 'gaussianSmoothing', SIGMA,
                                                          taps_fn=ctws.filter_taps))
