"""SizeFilterWorkflow: FindUniques(return_counts) -> SizeFilterBlocks -> BackgroundSizeFilter or
FillingSizeFilter -> RelabelWorkflow (cluster_tools/postprocess/postprocess_workflow.py:24-112).
An empty hmap_path selects the background filter.  The reference module's other workflows
(FilterLabels, FilterByThreshold, the graph-based ones) need node_labels, features and graph
first and are not part of this package."""
from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.relabel import RelabelWorkflow
from cluster_tools_amd.relabel import find_uniques as unique_tasks
from cluster_tools_amd.postprocess import size_filter_blocks as size_filter_tasks
from cluster_tools_amd.postprocess import background_size_filter as bg_tasks
from cluster_tools_amd.postprocess import filling_size_filter as filling_tasks


class SizeFilterWorkflow(WorkflowBase):
    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    size_threshold = luigi.IntParameter()
    hmap_path = luigi.Parameter(default='')
    hmap_key = luigi.Parameter(default='')
    relabel = luigi.BoolParameter(default=True)

    def _bg_filter(self, dep):
        filter_task = getattr(bg_tasks, self._get_task_name('BackgroundSizeFilter'))
        return filter_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                           input_path=self.input_path, input_key=self.input_key,
                           output_path=self.output_path, output_key=self.output_key, dependency=dep)

    def _ws_filter(self, dep):
        filter_task = getattr(filling_tasks, self._get_task_name('FillingSizeFilter'))
        return filter_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                           input_path=self.input_path, input_key=self.input_key,
                           output_path=self.output_path, output_key=self.output_key,
                           hmap_path=self.hmap_path, hmap_key=self.hmap_key, dependency=dep)

    def requires(self):
        un_task = getattr(unique_tasks, self._get_task_name('FindUniques'))
        dep = un_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                      input_path=self.input_path, input_key=self.input_key, return_counts=True,
                      dependency=self.dependency)
        sf_task = getattr(size_filter_tasks, self._get_task_name('SizeFilterBlocks'))
        dep = sf_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                      input_path=self.input_path, input_key=self.input_key, size_threshold=self.size_threshold,
                      dependency=dep)
        if self.hmap_path == '':
            assert self.hmap_key == ''
            dep = self._bg_filter(dep)
        else:
            assert self.hmap_key != ''
            dep = self._ws_filter(dep)
        if self.relabel:
            dep = RelabelWorkflow(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                                  target=self.target, input_path=self.output_path, input_key=self.output_key,
                                  assignment_path=self.output_path, assignment_key='relabel_size_filter',
                                  dependency=dep)
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'size_filter_blocks': size_filter_tasks.SizeFilterBlocksLocal.default_task_config(),
                        'background_size_filter': bg_tasks.BackgroundSizeFilterLocal.default_task_config(),
                        'filling_size_filter': filling_tasks.FillingSizeFilterLocal.default_task_config(),
                        **RelabelWorkflow.get_config()})
        return configs
