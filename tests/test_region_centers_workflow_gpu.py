"""RegionCentersWorkflow (target='local') end to end on the GPU on the small n5 volume of
tests/test_morphology_workflow_gpu.py (20 x 48 x 136 labels, blocks 8 x 16 x 64, maxId above the
largest id present: 2100 here, so that the ids fill two chunks of 2000, a job each) with one object
added that is one voxel thick.  The output equals the table of the restatement
(tests/region_centers_ref.py) on the volume and the workflow's own morphology table, exactly; every
non-zero centre lies inside its object."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import luigi_build

from cluster_tools_amd.utils import volume_utils as vu
import region_centers_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (20, 48, 136)
BLOCK_SHAPE = [8, 16, 64]
MAX_ID = 2100    # ids 62..2100 occur nowhere; two id chunks of 2000
SPRINKLED = 60
THIN = 61


@pytest.fixture(scope='module')
def volume():
    """A coarse random grid of the ids 0..49 enlarged to cells of 5 x 12 x 34 voxels, single voxels
    of id 60 sprinkled in, block (1, 1, 1) all zero, and a sheet of id 61 one voxel thick in z."""
    rng = np.random.RandomState(11)
    coarse = rng.randint(0, 50, (4, 4, 4)).astype(np.uint64)
    coarse[0, 0, 0] = coarse[3, 3, 3] = 0
    vol = np.ascontiguousarray(np.kron(coarse, np.ones((5, 12, 34), dtype=np.uint64)))
    assert vol.shape == SHAPE
    vol[rng.rand(*SHAPE) < .003] = SPRINKLED
    vol[8:16, 16:32, 64:128] = 0
    vol[17, 3:20, 5:40] = THIN
    return vol


def _run(tmp_path, vol, name, **kwargs):
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    from cluster_tools_amd.morphology.morphology_workflow import RegionCentersWorkflow
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
    out_path, tmp_folder = str(tmp_path / 'out.n5'), str(tmp_path / ('tmp_' + name))
    task = RegionCentersWorkflow(tmp_folder=tmp_folder, config_dir=str(cfg_dir), target='local', max_jobs=2,
                                 input_path=path, input_key='seg', output_path=out_path, output_key='centers_' + name,
                                 **kwargs)
    luigi_build(task, tmp_folder)
    with vu.file_reader(os.path.join(tmp_folder, 'region_centers.n5'), 'r') as f:
        morphology = f['morphology'][:]
    with vu.file_reader(out_path, 'r') as f:
        ds = f['centers_' + name]
        assert tuple(ds.shape) == (MAX_ID + 1, 3) and tuple(ds.chunks) == (2000, 3) and str(ds.dtype) == 'float32'
        got = ds[:]
    for n in ('region_centers.log', 'region_centers_job_0.config', 'region_centers_job_1.config',
              os.path.join('logs', 'region_centers_0.log'), os.path.join('logs', 'region_centers_1.log'),
              'block_morphology_region-centers.log', 'merge_morphology_region-centers.log'):
        assert os.path.exists(os.path.join(tmp_folder, n)), n
    return got, morphology


def _check(vol, got, morphology, ignore_label, resolution):
    assert got.dtype == np.float32 and morphology.shape == (MAX_ID + 1, 11)
    want = R.region_centers_table(vol, morphology, MAX_ID + 1, ignore_label, resolution)
    np.testing.assert_array_equal(got, want)
    present = np.unique(vol)
    nonzero = 0
    for i in range(MAX_ID + 1):
        if i not in present or i == THIN or i == ignore_label:
            assert not got[i].any(), i  # absent, one voxel thick, ignored: a zero row
            continue
        if got[i].any():
            nonzero += 1
            z, y, x = (int(c) for c in got[i])
            assert vol[z, y, x] == i, i  # the centre lies inside its object
    assert nonzero >= 30
    assert morphology[THIN, 1] == 17 * 35 and morphology[THIN, 5] == morphology[THIN, 8] == 17


def test_region_centers_workflow_default_resolution(tmp_path, volume):
    got, morphology = _run(tmp_path, volume, 'a')
    _check(volume, got, morphology, None, (1, 1, 1))
    # id 0 is an object like any other without ignore_label; its centre happens to be the volume's
    # first voxel (the corner cell, five voxels from the next cell in z), which reads like a zero row
    assert morphology[0, 1] > 0 and volume[0, 0, 0] == 0 and not got[0].any()


def test_region_centers_workflow_resolution_and_ignore_label(tmp_path, volume):
    got, morphology = _run(tmp_path, volume, 'b', resolution=[5, 1, 1], ignore_label=0)
    _check(volume, got, morphology, 0, (5, 1, 1))
    assert not got[0].any()
    # the anisotropic resolution moves some centre against the default's
    iso = R.region_centers_table(volume, morphology, MAX_ID + 1, 0, (1, 1, 1))
    assert (iso != got).any()
