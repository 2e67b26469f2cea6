"""NodeLabelWorkflow: BlockNodeLabels -> MergeNodeLabels
(cluster_tools/node_labels/node_label_workflow.py:8-59; parameters and config keys unchanged): for
every fragment the ids of a second label volume it overlaps, with the voxel counts, or the id of
the largest overlap.  The block overlaps go to `label_overlaps_<prefix>` in the output file."""
from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.node_labels import block_node_labels as label_tasks
from cluster_tools_amd.node_labels import merge_node_labels as merge_tasks


class NodeLabelWorkflow(WorkflowBase):
    ws_path = luigi.Parameter()
    ws_key = luigi.Parameter()
    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    prefix = luigi.Parameter(default='')
    max_overlap = luigi.BoolParameter(default=True)
    ignore_label = luigi.IntParameter(default=None)
    serialize_counts = luigi.BoolParameter(default=False)

    def requires(self):
        # (refused here too, so that no block job runs for a merge that cannot)
        merge_tasks.check_supported(self.max_overlap, self.serialize_counts)
        common = dict(max_jobs=self.max_jobs, tmp_folder=self.tmp_folder, config_dir=self.config_dir)
        tmp_key = 'label_overlaps_%s' % self.prefix
        label_task = getattr(label_tasks, self._get_task_name('BlockNodeLabels'))
        dep = label_task(dependency=self.dependency, ws_path=self.ws_path, ws_key=self.ws_key,
                         input_path=self.input_path, input_key=self.input_key, output_path=self.output_path,
                         output_key=tmp_key, ignore_label=self.ignore_label, prefix=self.prefix, **common)
        merge_task = getattr(merge_tasks, self._get_task_name('MergeNodeLabels'))
        dep = merge_task(dependency=dep, input_path=self.output_path, input_key=tmp_key,
                         output_path=self.output_path, output_key=self.output_key, max_overlap=self.max_overlap,
                         ignore_label=self.ignore_label, serialize_counts=self.serialize_counts,
                         prefix=self.prefix, **common)
        return dep

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'block_node_labels': label_tasks.BlockNodeLabelsLocal.default_task_config(),
                        'merge_node_labels': merge_tasks.MergeNodeLabelsLocal.default_task_config()})
        return configs
