"""The postprocessing workflows (cluster_tools/postprocess/postprocess_workflow.py).
SizeFilterWorkflow (:24-112): FindUniques(return_counts) -> SizeFilterBlocks -> BackgroundSizeFilter
or FillingSizeFilter -> RelabelWorkflow; an empty hmap_path selects the background filter.
ConnectedComponentsWorkflow (:296-339): GraphConnectedComponents [-> Write], the segments of an
assignment split where the fragment graph does not connect them.
SizeFilterAndGraphWatershedWorkflow (:342-427): FindUniques(return_counts) -> SizeFilterBlocks ->
GraphWatershedAssignments [-> Write], every segment below size_threshold voxels merged into a
neighbour along the cheapest graph edges.  The Write step runs when output_key is given and needs
fragments_key.  The reference module's FilterLabels, FilterByThreshold and FilterOrphans workflows
are not part of this package."""
import os

from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.relabel import RelabelWorkflow
from cluster_tools_amd.relabel import find_uniques as unique_tasks
from cluster_tools_amd.postprocess import size_filter_blocks as size_filter_tasks
from cluster_tools_amd.postprocess import background_size_filter as bg_tasks
from cluster_tools_amd.postprocess import filling_size_filter as filling_tasks
from cluster_tools_amd.postprocess import graph_connected_components as cc_tasks
from cluster_tools_amd.postprocess import graph_watershed_assignments as gws_tasks
from cluster_tools_amd import write as write_tasks


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


class ConnectedComponentsWorkflow(WorkflowBase):
    problem_path = luigi.Parameter()
    graph_key = luigi.Parameter()

    path = luigi.Parameter()
    fragments_key = luigi.Parameter(default='')
    assignment_path = luigi.Parameter()
    assignment_key = luigi.Parameter()

    output_path = luigi.Parameter()
    assignment_out_key = luigi.Parameter()
    output_key = luigi.Parameter(default='')

    def requires(self):
        cc_task = getattr(cc_tasks, self._get_task_name('GraphConnectedComponents'))
        dep = cc_task(max_jobs=self.max_jobs, tmp_folder=self.tmp_folder, config_dir=self.config_dir,
                      problem_path=self.problem_path, graph_key=self.graph_key,
                      assignment_path=self.assignment_path, assignment_key=self.assignment_key,
                      output_path=self.output_path, output_key=self.assignment_out_key, dependency=self.dependency)
        if self.output_key != '':
            write_task = getattr(write_tasks, self._get_task_name('Write'))
            assert self.fragments_key != ''
            dep = write_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                             dependency=dep, input_path=self.path, input_key=self.fragments_key,
                             output_path=self.output_path, output_key=self.output_key,
                             assignment_path=self.output_path, assignment_key=self.assignment_out_key,
                             identifier='graph-connected-components')
        return dep

    @staticmethod
    def get_config():
        # (the reference's get_config calls functions that do not exist)
        configs = WorkflowBase.get_config()
        configs.update({'graph_connected_components': cc_tasks.GraphConnectedComponentsLocal.default_task_config(),
                        'write': write_tasks.WriteLocal.default_task_config()})
        return configs


class SizeFilterAndGraphWatershedWorkflow(WorkflowBase):
    problem_path = luigi.Parameter()
    graph_key = luigi.Parameter()
    features_key = luigi.Parameter()

    path = luigi.Parameter()
    # the merged segmentation
    segmentation_key = luigi.Parameter()
    # the underlying fragments
    fragments_key = luigi.Parameter(default='')
    # the fragment-segment assignment
    assignment_key = luigi.Parameter()

    size_threshold = luigi.IntParameter()
    relabel = luigi.BoolParameter(default=False)
    from_costs = luigi.BoolParameter(default=False)

    output_path = luigi.Parameter()
    assignment_out_key = luigi.Parameter()
    output_key = luigi.Parameter(default='')

    def find_sizes(self, dep):
        # the segments that the size filter discards: discard_ids.npy in tmp_folder
        un_task = getattr(unique_tasks, self._get_task_name('FindUniques'))
        dep = un_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                      input_path=self.path, input_key=self.segmentation_key, return_counts=True, dependency=dep)
        sf_task = getattr(size_filter_tasks, self._get_task_name('SizeFilterBlocks'))
        return sf_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                       input_path=self.path, input_key=self.segmentation_key, size_threshold=self.size_threshold,
                       dependency=dep)

    def requires(self):
        dep = self.find_sizes(self.dependency)
        filter_path = os.path.join(self.tmp_folder, 'discard_ids.npy')
        gws_task = getattr(gws_tasks, self._get_task_name('GraphWatershedAssignments'))
        dep = gws_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir, dependency=dep,
                       problem_path=self.problem_path, graph_key=self.graph_key, features_key=self.features_key,
                       assignment_path=self.path, assignment_key=self.assignment_key,
                       output_path=self.output_path, output_key=self.assignment_out_key,
                       filter_nodes_path=filter_path, relabel=self.relabel, from_costs=self.from_costs)
        if self.output_key != '':
            assert self.fragments_key != ''
            write_task = getattr(write_tasks, self._get_task_name('Write'))
            dep = write_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                             dependency=dep, input_path=self.path, input_key=self.fragments_key,
                             output_path=self.output_path, output_key=self.output_key,
                             assignment_path=self.output_path, assignment_key=self.assignment_out_key,
                             identifier='size-filter-graph-ws')
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'find_uniques': unique_tasks.FindUniquesLocal.default_task_config(),
                        'size_filter_blocks': size_filter_tasks.SizeFilterBlocksLocal.default_task_config(),
                        'graph_watershed_assignments':
                        gws_tasks.GraphWatershedAssignmentsLocal.default_task_config(),
                        'write': write_tasks.WriteLocal.default_task_config()})
        return configs
