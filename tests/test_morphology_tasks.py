"""CPU tests of the MorphologyWorkflow task surface (cluster_tools/morphology/
morphology_workflow.py:11-56, block_morphology.py, merge_morphology.py): class names, parameters,
config keys, job and log names, the task graph, the missing-maxId error, and MergeMorphologyLocal
run on block chunks written from the restatement (tests/morphology_ref.py).  No GPU call is made."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import luigi_build

from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import _Paths, BaseClusterTask, DummyTask
from cluster_tools_amd.io import File
from cluster_tools_amd.morphology import MorphologyWorkflow
from cluster_tools_amd.morphology import block_morphology as block
from cluster_tools_amd.morphology import merge_morphology as merge
from cluster_tools_amd.morphology import serialization as S
from cluster_tools_amd.utils import volume_utils as vu
from cluster_tools_amd.utils.blocking import Blocking
import cluster_tools_amd.morphology as package
import morphology_ref as R

COMMON = {'threads_per_job': 1, 'time_limit': 60, 'mem_limit': 1., 'qos': 'normal'}
TASK = ['tmp_folder', 'max_jobs', 'config_dir']


def _names(cls):
    return [n for n, _ in cls.get_params()]


def test_task_names_and_parameters():
    assert block.BlockMorphologyLocal.task_name == 'block_morphology'
    assert merge.MergeMorphologyLocal.task_name == 'merge_morphology'
    assert merge.MergeMorphologyLocal.allow_retry is False and block.BlockMorphologyLocal.allow_retry is True
    for mod, base in ((block, 'BlockMorphology'), (merge, 'MergeMorphology')):
        for target in ('Base', 'Local', 'Slurm', 'LSF'):
            assert hasattr(mod, base + target)
    assert sorted(_names(block.BlockMorphologyLocal)) == sorted(
        TASK + ['input_path', 'input_key', 'output_path', 'output_key', 'prefix', 'dependency'])
    assert sorted(_names(merge.MergeMorphologyLocal)) == sorted(
        TASK + ['input_path', 'input_key', 'output_path', 'output_key', 'number_of_labels', 'prefix', 'dependency'])
    assert sorted(_names(MorphologyWorkflow)) == sorted(
        TASK + ['target', 'dependency', 'input_path', 'input_key', 'output_path', 'output_key', 'max_jobs_merge',
                'prefix'])
    if not luigi.HAVE_LUIGI:
        d = {n: p.default for n, p in MorphologyWorkflow.get_params() if n in ('prefix', 'max_jobs_merge')}
        assert d == {'prefix': '', 'max_jobs_merge': None}
    # RegionCentersWorkflow is not built
    assert not hasattr(package, 'RegionCentersWorkflow')


def test_config_keys():
    assert block.BlockMorphologyLocal.default_task_config() == COMMON
    assert merge.MergeMorphologyLocal.default_task_config() == COMMON
    cfg = MorphologyWorkflow.get_config()
    assert sorted(cfg) == ['block_morphology', 'global', 'merge_morphology']
    assert cfg['block_morphology'] == COMMON and cfg['merge_morphology'] == COMMON


def _input(tmp_path, max_id=41):
    path = str(tmp_path / 'seg.n5')
    ds = File(path).create_dataset('seg', data=np.ones((4, 4, 4), 'uint64'), chunks=(4, 4, 4))
    if max_id is not None:
        ds.attrs['maxId'] = max_id
    return path


def _workflow(path, **kwargs):
    args = dict(tmp_folder='tmp', max_jobs=3, config_dir='cfg', target='local', input_path=path, input_key='seg',
                output_path='out.n5', output_key='morphology')
    args.update(kwargs)
    return MorphologyWorkflow(**args)


@pytest.mark.parametrize('prefix', ['', 'seg'])
def test_task_graph_and_log_names(tmp_path, prefix):
    path = _input(tmp_path)
    m = _workflow(path, prefix=prefix, target='slurm').requires()
    b = m.requires()
    assert type(m).__name__ == 'MergeMorphologySlurm' and type(b).__name__ == 'BlockMorphologySlurm'
    assert isinstance(b, luigi.Task) and isinstance(b.requires(), DummyTask)
    # the block tables go to morphology_<prefix> of the output file, the merge reads them there
    assert (b.input_path, b.input_key, b.output_path, b.output_key, b.prefix, b.max_jobs) \
        == (path, 'seg', 'out.n5', 'morphology_%s' % prefix, prefix, 3)
    assert (m.input_path, m.input_key, m.output_path, m.output_key, m.number_of_labels, m.prefix, m.max_jobs) \
        == ('out.n5', 'morphology_%s' % prefix, 'out.n5', 'morphology', 42, prefix, 3)
    # task logs (the luigi targets), job configs and job logs
    assert b.output().path == os.path.join('tmp', 'block_morphology_%s.log' % prefix)
    assert m.output().path == os.path.join('tmp', 'merge_morphology_%s.log' % prefix)
    p = _Paths('tmp', b.task_name, b.prefix)
    assert p.config(1) == os.path.join('tmp', 'block_morphology_job_%s_1.config' % prefix)
    assert p.log(1) == os.path.join('tmp', 'logs', 'block_morphology_%s_1.log' % prefix)
    p = _Paths('tmp', m.task_name, m.prefix)
    assert p.config(0) == os.path.join('tmp', 'merge_morphology_job_%s_0.config' % prefix)


def test_max_jobs_merge(tmp_path):
    path = _input(tmp_path)
    assert _workflow(path).requires().max_jobs == 3  # the default: max_jobs
    m = _workflow(path, max_jobs_merge=7).requires()
    assert m.max_jobs == 7 and m.requires().max_jobs == 3


def test_missing_max_id(tmp_path):
    path = _input(tmp_path, max_id=None)
    with pytest.raises(KeyError, match='Dataset %s:seg does not have attribute maxId' % path):
        _workflow(path).requires()


# ids of the merge test: three label ranges of 100000, an id at both ends of a range
IDS = np.array([0, 1, 2, 3, 99999, 100000, 150000, 200499], dtype=np.uint64)
N_LABELS = 200600
SHAPE, BLOCK_SHAPE = (10, 12, 20), [4, 8, 8]
UNWRITTEN = 7


@pytest.fixture(scope='module')
def block_tables():
    rng = np.random.RandomState(0)
    coarse = rng.randint(0, len(IDS), (5, 4, 5))
    vol = IDS[np.kron(coarse, np.ones((2, 3, 4), dtype=np.int64))]
    assert vol.shape == SHAPE and len(np.unique(vol)) == len(IDS)
    blocking = Blocking([0, 0, 0], list(SHAPE), BLOCK_SHAPE)
    assert blocking.numberOfBlocks == 18
    tables = []
    for block_id in range(blocking.numberOfBlocks):
        b = blocking.getBlock(block_id)
        cid = tuple(beg // bs for beg, bs in zip(b.begin, BLOCK_SHAPE))
        tables.append((cid, R.block_morphology(vol[vu.block_to_bb(b)], b.begin)))
    return tables


def _run_merge(tmp_path, tables, number_of_labels, max_jobs):
    cfg_dir = tmp_path / 'configs'
    cfg_dir.mkdir()
    g = BaseClusterTask.default_global_config()
    g['shebang'] = '#! ' + sys.executable
    (cfg_dir / 'global.config').write_text(json.dumps(g))
    path, tmp_folder = str(tmp_path / 'out.n5'), str(tmp_path / 'tmp')
    with vu.file_reader(path) as f:
        ds = f.require_dataset('morphology_', shape=SHAPE, dtype='float64', chunks=tuple(BLOCK_SHAPE),
                               compression='gzip')
        for k, (cid, t) in enumerate(tables):
            if k != UNWRITTEN:
                ds.write_chunk(cid, S.serialize_morphology(t), True)
    task = merge.MergeMorphologyLocal(tmp_folder=tmp_folder, max_jobs=max_jobs, config_dir=str(cfg_dir),
                                      input_path=path, input_key='morphology_', output_path=path,
                                      output_key='morphology', number_of_labels=number_of_labels, prefix='',
                                      dependency=DummyTask())
    luigi_build(task, tmp_folder)
    return path, tmp_folder


@pytest.mark.parametrize('max_jobs', [1, 3])
def test_merge_task(tmp_path, block_tables, max_jobs):
    path, tmp_folder = _run_merge(tmp_path, block_tables, N_LABELS, max_jobs)
    want = R.merge_morphology(N_LABELS, [t for k, (_, t) in enumerate(block_tables) if k != UNWRITTEN])
    with vu.file_reader(path, 'r') as f:
        ds = f['morphology']
        assert tuple(ds.shape) == (N_LABELS, 11) and tuple(ds.chunks) == (100000, 11) and str(ds.dtype) == 'float64'
        got = ds[:]
    np.testing.assert_array_equal(got, want)
    present = np.zeros(N_LABELS, dtype=bool)
    present[IDS.astype(np.int64)] = True
    assert not got[~present].any()  # an id that occurs nowhere: eleven zeros
    assert (got[present, 1] > 0).all() and got[0, 0] == 0
    np.testing.assert_array_equal(got[present, 0], IDS.astype(np.float64))
    # the unwritten block's voxels are missing from the sizes, nothing else
    assert got[:, 1].sum() == np.prod(SHAPE) - block_tables[UNWRITTEN][1][:, 1].sum()
    # the label ranges are dealt to max_jobs jobs
    cfgs = [json.load(open(_Paths(tmp_folder, 'merge_morphology', '').config(j))) for j in range(max_jobs)]
    assert sorted(b for c in cfgs for b in c['block_list']) == [0, 1, 2]
    assert cfgs[0]['out_shape'] == [N_LABELS, 11] and cfgs[0]['out_chunks'] == [100000, 11]
    assert os.path.exists(os.path.join(tmp_folder, 'merge_morphology_.log'))


def test_merge_task_refuses_an_id_out_of_range(tmp_path, block_tables):
    with pytest.raises(AssertionError, match=r'RuntimeError: merge_morphology: id 200499 in chunk \(\d, \d, \d\)'):
        _run_merge(tmp_path, block_tables, 200499, 1)
