"""CPU tests of the EdgeFeaturesWorkflow task surface (cluster_tools/features/features_workflow.py:
14-66, block_edge_features.py, merge_edge_features.py): class names, parameters, config keys, the
input check, the refusal of the filter and affinity paths, the task graph and the host merge
against the restatement (tests/edge_features_ref.py).  No GPU call is made."""
import json

import numpy as np
import pytest

from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.features import EdgeFeaturesWorkflow
from cluster_tools_amd.features import block_edge_features as feat
from cluster_tools_amd.features import merge_edge_features as merge
import edge_features_ref as E

COMMON = {'threads_per_job': 1, 'time_limit': 60, 'mem_limit': 1., 'qos': 'normal'}


def _names(cls):
    return [n for n, _ in cls.get_params()]


def test_task_names_and_parameters():
    common = ['tmp_folder', 'max_jobs', 'config_dir']
    assert feat.BlockEdgeFeaturesLocal.task_name == 'block_edge_features'
    assert merge.MergeEdgeFeaturesLocal.task_name == 'merge_edge_features'
    assert merge.MergeEdgeFeaturesLocal.allow_retry is False and feat.BlockEdgeFeaturesLocal.allow_retry is True
    for mod, base in ((feat, 'BlockEdgeFeatures'), (merge, 'MergeEdgeFeatures')):
        for target in ('Base', 'Local', 'Slurm', 'LSF'):
            assert hasattr(mod, base + target)
    assert sorted(_names(feat.BlockEdgeFeaturesLocal)) == sorted(
        common + ['input_path', 'input_key', 'labels_path', 'labels_key', 'graph_path', 'output_path', 'dependency'])
    assert sorted(_names(merge.MergeEdgeFeaturesLocal)) == sorted(
        common + ['graph_path', 'graph_key', 'output_path', 'output_key', 'dependency'])
    assert sorted(_names(EdgeFeaturesWorkflow)) == sorted(
        common + ['target', 'dependency', 'input_path', 'input_key', 'labels_path', 'labels_key', 'graph_path',
                  'graph_key', 'output_path', 'output_key', 'max_jobs_merge'])


def test_config_keys():
    assert feat.BlockEdgeFeaturesLocal.default_task_config() == dict(
        COMMON, offsets=None, filters=None, sigmas=None, halo=[0, 0, 0], apply_in_2d=False,
        channel_agglomeration='mean')
    assert merge.MergeEdgeFeaturesLocal.default_task_config() == COMMON
    cfg = EdgeFeaturesWorkflow.get_config()
    assert sorted(cfg) == ['block_edge_features', 'global', 'merge_edge_features']
    assert cfg['block_edge_features'] == feat.BlockEdgeFeaturesLocal.default_task_config()


def test_check_input_rejects_h5():
    for ok in ('a.n5', 'b.zarr', 'c.ZR'):
        EdgeFeaturesWorkflow._check_input(ok)
    with pytest.raises(AssertionError, match='Only support n5 and zarr'):
        EdgeFeaturesWorkflow._check_input('labels.h5')
    wf = EdgeFeaturesWorkflow(tmp_folder='tmp', max_jobs=2, config_dir='cfg', target='local', input_path='a.n5',
                              input_key='bmap', labels_path='seg.h5', labels_key='seg', graph_path='g.n5',
                              graph_key='graph', output_path='f.n5', output_key='features')
    with pytest.raises(AssertionError):
        wf.requires()


@pytest.mark.parametrize('key,value', [('filters', ['gaussianSmoothing']), ('sigmas', [1.6]),
                                       ('offsets', [[-1, 0, 0], [0, -1, 0], [0, 0, -1]])])
def test_filter_and_affinity_paths_are_refused(tmp_path, key, value):
    config = feat.BlockEdgeFeaturesLocal.default_task_config()
    feat.check_supported(config)
    config[key] = value
    with pytest.raises(NotImplementedError, match=key):
        feat.check_supported(config)
    # the job refuses before it opens anything (the paths do not exist)
    config.update({'block_list': [0], 'input_path': str(tmp_path / 'no.n5'), 'input_key': 'x',
                   'labels_path': str(tmp_path / 'no.n5'), 'labels_key': 'y', 'output_path': str(tmp_path / 'o.n5'),
                   'block_shape': [8, 8, 8], 'graph_block_prefix': str(tmp_path / 'g.n5/s0/sub_graphs/block_')})
    path = tmp_path / 'block_edge_features_job_0.config'
    path.write_text(json.dumps(config))
    with pytest.raises(NotImplementedError, match=key):
        feat.block_edge_features(0, str(path))


def test_workflow_task_graph():
    wf = EdgeFeaturesWorkflow(tmp_folder='tmp', max_jobs=3, config_dir='cfg', target='slurm', input_path='a.n5',
                              input_key='bmap', labels_path='s.zarr', labels_key='seg', graph_path='g.n5',
                              graph_key='graph', output_path='f.n5', output_key='features', max_jobs_merge=2)
    m = wf.requires()
    b = m.requires()
    assert type(m).__name__ == 'MergeEdgeFeaturesSlurm' and type(b).__name__ == 'BlockEdgeFeaturesSlurm'
    assert isinstance(b, luigi.Task) and m.max_jobs == 2 and b.max_jobs == 3
    assert (m.graph_path, m.graph_key, m.output_path, m.output_key) == ('g.n5', 'graph', 'f.n5', 'features')
    assert (b.input_path, b.input_key, b.labels_path, b.labels_key, b.graph_path, b.output_path) == \
        ('a.n5', 'bmap', 's.zarr', 'seg', 'g.n5', 'f.n5')
    assert EdgeFeaturesWorkflow(tmp_folder='tmp', max_jobs=3, config_dir='cfg', target='local', input_path='a.n5',
                                input_key='bmap', labels_path='s.n5', labels_key='seg', graph_path='g.n5',
                                graph_key='graph', output_path='f.n5', output_key='f').max_jobs_merge == 1


def test_host_merge_equals_the_restated_merge():
    rng = np.random.default_rng(3)
    n_edges, blocks = 40, []
    for _ in range(6):
        ids = np.sort(rng.choice(n_edges - 3, size=12, replace=False))  # the last three edges get no row
        feats = np.sort(rng.random((12, 10)), axis=1)
        feats[:, 9] = rng.integers(0, 5, 12)
        feats[feats[:, 9] == 0] = 0
        blocks.append((ids, feats))
    ref = E.merge_features(n_edges, blocks)
    ids, rows = np.concatenate([b[0] for b in blocks]), np.concatenate([b[1] for b in blocks])
    np.testing.assert_array_equal(merge.merge_feature_rows(ids, rows, 0, n_edges), ref)
    # a job's edge range: only its rows, whatever the other ranges hold
    np.testing.assert_array_equal(merge.merge_feature_rows(ids, rows, 7, 29), ref[7:29])
    assert not ref[-3:].any() and (ref[:, 9] > 0).sum() > 20
