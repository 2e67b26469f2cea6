"""EdgeFeaturesWorkflow: BlockEdgeFeatures -> MergeEdgeFeatures
(cluster_tools/features/features_workflow.py:14-66; parameters and config keys unchanged), and
RegionFeaturesWorkflow: RegionFeatures -> MergeRegionFeatures (:71-112, likewise): the
(maxId + 1,) float32 table of every fragment's mean input value."""
from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.features import block_edge_features as feat_tasks
from cluster_tools_amd.features import merge_edge_features as merge_tasks
from cluster_tools_amd.features import region_features as reg_tasks
from cluster_tools_amd.features import merge_region_features as merge_reg_tasks
from cluster_tools_amd.utils import volume_utils as vu


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


class RegionFeaturesWorkflow(WorkflowBase):
    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    labels_path = luigi.Parameter()
    labels_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()

    def read_number_of_labels(self):
        with vu.file_reader(self.labels_path, 'r') as f:
            try:
                return int(f[self.labels_key].attrs['maxId']) + 1
            except KeyError:
                raise KeyError("Dataset %s:%s does not have attribute maxId" % (self.labels_path, self.labels_key))

    def requires(self):
        common = dict(tmp_folder=self.tmp_folder, config_dir=self.config_dir, max_jobs=self.max_jobs)
        feat_task = getattr(reg_tasks, self._get_task_name('RegionFeatures'))
        dep = feat_task(input_path=self.input_path, input_key=self.input_key, labels_path=self.labels_path,
                        labels_key=self.labels_key, dependency=self.dependency, **common)
        merge_task = getattr(merge_reg_tasks, self._get_task_name('MergeRegionFeatures'))
        dep = merge_task(output_path=self.output_path, output_key=self.output_key,
                         number_of_labels=self.read_number_of_labels(), dependency=dep, **common)
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'region_features': reg_tasks.RegionFeaturesLocal.default_task_config(),
                        'merge_region_features': merge_reg_tasks.MergeRegionFeaturesLocal.default_task_config()})
        return configs
