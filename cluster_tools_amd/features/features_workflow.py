"""EdgeFeaturesWorkflow: BlockEdgeFeatures -> MergeEdgeFeatures
(cluster_tools/features/features_workflow.py:14-66; parameters and config keys unchanged).  The
reference's RegionFeaturesWorkflow (:71-112) is not built here."""
from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.features import block_edge_features as feat_tasks
from cluster_tools_amd.features import merge_edge_features as merge_tasks


class EdgeFeaturesWorkflow(WorkflowBase):
    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    labels_path = luigi.Parameter()
    labels_key = luigi.Parameter()
    graph_path = luigi.Parameter()
    graph_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    max_jobs_merge = luigi.IntParameter(default=1)

    # only n5 / zarr inputs, as the reference
    @staticmethod
    def _check_input(path):
        ending = path.split('.')[-1]
        assert ending.lower() in ('zr', 'zarr', 'n5'), "Only support n5 and zarr files, not %s" % ending

    def requires(self):
        self._check_input(self.input_path)
        self._check_input(self.labels_path)
        common = dict(tmp_folder=self.tmp_folder, config_dir=self.config_dir)
        feat_task = getattr(feat_tasks, self._get_task_name('BlockEdgeFeatures'))
        dep = feat_task(max_jobs=self.max_jobs, input_path=self.input_path, input_key=self.input_key,
                        labels_path=self.labels_path, labels_key=self.labels_key, graph_path=self.graph_path,
                        output_path=self.output_path, dependency=self.dependency, **common)
        merge_task = getattr(merge_tasks, self._get_task_name('MergeEdgeFeatures'))
        dep = merge_task(max_jobs=self.max_jobs_merge, graph_path=self.graph_path, graph_key=self.graph_key,
                         output_path=self.output_path, output_key=self.output_key, dependency=dep, **common)
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'block_edge_features': feat_tasks.BlockEdgeFeaturesLocal.default_task_config(),
                        'merge_edge_features': merge_tasks.MergeEdgeFeaturesLocal.default_task_config()})
        return configs
