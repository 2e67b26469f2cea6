"""CPU tests of the RegionFeaturesWorkflow task surface (cluster_tools/features/
features_workflow.py:71-112, region_features.py, merge_region_features.py): class names,
parameters, config keys, the task graph, the missing-maxId error, the refusal of a 4-D input, and
MergeRegionFeaturesLocal run on block chunks written from the restatement
(tests/region_features_ref.py).  No GPU call is made."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import luigi_build

from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import _Paths, BaseClusterTask, DummyTask
from cluster_tools_amd.io import File
from cluster_tools_amd.features import RegionFeaturesWorkflow
from cluster_tools_amd.features import region_features as reg
from cluster_tools_amd.features import merge_region_features as merge
from cluster_tools_amd.features import region_serialization as S
from cluster_tools_amd.utils import volume_utils as vu
from cluster_tools_amd.utils.blocking import Blocking
import cluster_tools_amd.features as package
import region_features_ref as R

COMMON = {'threads_per_job': 1, 'time_limit': 60, 'mem_limit': 1., 'qos': 'normal'}
TASK = ['tmp_folder', 'max_jobs', 'config_dir']


def _names(cls):
    return [n for n, _ in cls.get_params()]


def test_task_names_and_parameters():
    assert reg.RegionFeaturesLocal.task_name == 'region_features'
    assert merge.MergeRegionFeaturesLocal.task_name == 'merge_region_features'
    assert merge.MergeRegionFeaturesLocal.allow_retry is False and reg.RegionFeaturesLocal.allow_retry is True
    for mod, base in ((reg, 'RegionFeatures'), (merge, 'MergeRegionFeatures')):
        for target in ('Base', 'Local', 'Slurm', 'LSF'):
            assert hasattr(mod, base + target)
    assert sorted(_names(reg.RegionFeaturesLocal)) == sorted(
        TASK + ['input_path', 'input_key', 'labels_path', 'labels_key', 'dependency'])
    assert sorted(_names(merge.MergeRegionFeaturesLocal)) == sorted(
        TASK + ['output_path', 'output_key', 'number_of_labels', 'dependency'])
    assert sorted(_names(RegionFeaturesWorkflow)) == sorted(
        TASK + ['target', 'dependency', 'input_path', 'input_key', 'labels_path', 'labels_key', 'output_path',
                'output_key'])
    assert hasattr(package, 'EdgeFeaturesWorkflow') and hasattr(package, 'RegionFeaturesWorkflow')


def test_config_keys():
    assert reg.RegionFeaturesLocal.default_task_config() == dict(COMMON, ignore_label=0)
    assert merge.MergeRegionFeaturesLocal.default_task_config() == COMMON
    cfg = RegionFeaturesWorkflow.get_config()
    assert sorted(cfg) == ['global', 'merge_region_features', 'region_features']
    assert cfg['region_features'] == dict(COMMON, ignore_label=0) and cfg['merge_region_features'] == COMMON


def test_serialization_round_trip():
    rows = np.array([[0., 0., 0.], [2. ** 40, 5., .25]])
    flat = S.serialize_region_features(rows)
    assert flat.dtype == np.float64 and flat.shape == (6,)
    assert flat[::3].tolist() == [0., 2. ** 40] and flat[1::3].tolist() == [0., 5.] and flat[2::3].tolist() == [0., .25]
    np.testing.assert_array_equal(S.deserialize_region_features(flat), rows)
    with pytest.raises(ValueError):
        S.deserialize_region_features(np.zeros(4))
    with pytest.raises(ValueError):
        S.serialize_region_features(np.zeros((2, 4)))


def _labels(tmp_path, max_id=41):
    path = str(tmp_path / 'seg.n5')
    f = File(path)
    ds = f.create_dataset('seg', data=np.ones((4, 4, 4), 'uint64'), chunks=(4, 4, 4))
    f.create_dataset('raw', data=np.ones((4, 4, 4), 'float32'), chunks=(4, 4, 4))
    f.create_dataset('affs', data=np.ones((3, 4, 4, 4), 'float32'), chunks=(1, 4, 4, 4))
    if max_id is not None:
        ds.attrs['maxId'] = max_id
    return path


def _workflow(path, **kwargs):
    args = dict(tmp_folder='tmp', max_jobs=3, config_dir='cfg', target='local', input_path=path, input_key='raw',
                labels_path=path, labels_key='seg', output_path='out.n5', output_key='feats')
    args.update(kwargs)
    return RegionFeaturesWorkflow(**args)


def test_task_graph(tmp_path):
    path = _labels(tmp_path)
    m = _workflow(path, target='slurm').requires()
    b = m.requires()
    assert type(m).__name__ == 'MergeRegionFeaturesSlurm' and type(b).__name__ == 'RegionFeaturesSlurm'
    assert isinstance(b, luigi.Task) and isinstance(b.requires(), DummyTask)
    assert (b.input_path, b.input_key, b.labels_path, b.labels_key, b.max_jobs) == (path, 'raw', path, 'seg', 3)
    assert (m.output_path, m.output_key, m.number_of_labels, m.max_jobs) == ('out.n5', 'feats', 42, 3)
    p = _Paths('tmp', b.task_name, None)
    assert p.config(1) == os.path.join('tmp', 'region_features_job_1.config')


def test_missing_max_id(tmp_path):
    path = _labels(tmp_path, max_id=None)
    with pytest.raises(KeyError, match='Dataset %s:seg does not have attribute maxId' % path):
        _workflow(path).requires()


def test_a_4d_input_is_refused_before_any_job(tmp_path):
    path = _labels(tmp_path)
    cfg_dir = tmp_path / 'configs'
    cfg_dir.mkdir()
    g = BaseClusterTask.default_global_config()
    g['shebang'] = '#! ' + sys.executable
    (cfg_dir / 'global.config').write_text(json.dumps(g))
    tmp_folder = str(tmp_path / 'tmp')
    task = reg.RegionFeaturesLocal(tmp_folder=tmp_folder, max_jobs=1, config_dir=str(cfg_dir), input_path=path,
                                   input_key='affs', labels_path=path, labels_key='seg', dependency=DummyTask())
    with pytest.raises(NotImplementedError, match='multi-channel'):
        task.run()
    assert not os.path.exists(_Paths(tmp_folder, 'region_features', None).config(0))


# ids of the merge test: three label ranges of 10000, an id at both ends of a range
IDS = np.array([0, 1, 2, 3, 9999, 10000, 15000, 24999], dtype=np.uint64)
N_LABELS = 25100
SHAPE, BLOCK_SHAPE = (10, 12, 20), [4, 8, 8]
UNWRITTEN = 7


@pytest.fixture(scope='module')
def block_tables():
    rng = np.random.RandomState(0)
    coarse = rng.randint(0, len(IDS), (5, 4, 5))
    vol = IDS[np.kron(coarse, np.ones((2, 3, 4), dtype=np.int64))]
    assert vol.shape == SHAPE and len(np.unique(vol)) == len(IDS)
    data = rng.rand(*SHAPE).astype('float32')
    blocking = Blocking([0, 0, 0], list(SHAPE), BLOCK_SHAPE)
    assert blocking.numberOfBlocks == 18
    tables = []
    for block_id in range(blocking.numberOfBlocks):
        b = blocking.getBlock(block_id)
        cid = tuple(beg // bs for beg, bs in zip(b.begin, BLOCK_SHAPE))
        bb = vu.block_to_bb(b)
        tables.append((cid, R.block_rows(vol[bb], data[bb], 0)))
    return tables


def _run_merge(tmp_path, tables, number_of_labels, max_jobs):
    cfg_dir = tmp_path / 'configs'
    cfg_dir.mkdir()
    g = BaseClusterTask.default_global_config()
    g['shebang'] = '#! ' + sys.executable
    (cfg_dir / 'global.config').write_text(json.dumps(g))
    path, tmp_folder = str(tmp_path / 'out.n5'), str(tmp_path / 'tmp')
    os.makedirs(tmp_folder)
    with vu.file_reader(os.path.join(tmp_folder, 'region_features_tmp.n5')) as f:
        ds = f.require_dataset('block_feats', shape=SHAPE, dtype='float64', chunks=tuple(BLOCK_SHAPE),
                               compression='gzip')
        for k, (cid, t) in enumerate(tables):
            if k != UNWRITTEN:
                ds.write_chunk(cid, S.serialize_region_features(t), True)
    task = merge.MergeRegionFeaturesLocal(tmp_folder=tmp_folder, max_jobs=max_jobs, config_dir=str(cfg_dir),
                                          output_path=path, output_key='feats', number_of_labels=number_of_labels,
                                          dependency=DummyTask())
    luigi_build(task, tmp_folder)
    return path, tmp_folder


@pytest.mark.parametrize('max_jobs', [1, 3])
def test_merge_task(tmp_path, block_tables, max_jobs):
    path, tmp_folder = _run_merge(tmp_path, block_tables, N_LABELS, max_jobs)
    written = [t for k, (_, t) in enumerate(block_tables) if k != UNWRITTEN]
    want = R.merge(N_LABELS, written)
    with vu.file_reader(path, 'r') as f:
        ds = f['feats']
        assert tuple(ds.shape) == (N_LABELS,) and tuple(ds.chunks) == (10000,) and str(ds.dtype) == 'float32'
        got = ds[:]
    np.testing.assert_array_equal(got, want)
    assert np.allclose(got, R.merge_running_average(N_LABELS, written))
    present = np.zeros(N_LABELS, dtype=bool)
    present[IDS.astype(np.int64)] = True
    assert not got[~present].any()  # an id that occurs nowhere: 0
    assert got[0] == 0              # the ignore label: 0
    present[0] = False
    assert (got[present] > 0).all()
    # the label ranges are dealt consecutively to max_jobs jobs
    cfgs = [json.load(open(_Paths(tmp_folder, 'merge_region_features', None).config(j))) for j in range(max_jobs)]
    assert [c['block_list'] for c in cfgs] == ([[0, 1, 2]] if max_jobs == 1 else [[0], [1], [2]])
    assert cfgs[0]['node_chunk_size'] == 10000 and cfgs[0]['tmp_key'] == 'block_feats'
    assert cfgs[0]['tmp_path'] == os.path.join(tmp_folder, 'region_features_tmp.n5')
    assert os.path.exists(os.path.join(tmp_folder, 'merge_region_features.log'))


def test_merge_task_refuses_an_id_out_of_range(tmp_path, block_tables):
    with pytest.raises(AssertionError,
                       match=r'RuntimeError: merge_region_features: id 24999 in chunk \(\d, \d, \d\)'):
        _run_merge(tmp_path, block_tables, 24999, 1)
