"""LiftedFeaturesFromNodeLabelsWorkflow: NodeLabelWorkflow -> SparseLiftedNeighborhood
[-> NodeLabelWorkflow(clear labels) -> ClearLiftedEdgesFromLabels] -> CostsFromNodeLabels
(cluster_tools/lifted_features/lifted_feature_workflow.py:80-198; parameters, dataset keys
node_overlaps/<prefix> and node_overlaps/clear_<prefix>, and config keys unchanged).  The front half
of the lifted multicut: the fragments' labels under a second segmentation, the pairs of labelled
fragments at most nh_graph_depth hops apart that no graph edge joins, and an attractive or
repulsive cost for each.

label_overlap_threshold needs the overlap counts of every node (serialize_counts), which
NodeLabelWorkflow refuses together with its 1-D output; NodeLabelsWithThreshold is not ported and the
workflow refuses the parameter before anything runs."""
from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.node_labels import NodeLabelWorkflow
from cluster_tools_amd.lifted_features import sparse_lifted_neighborhood as nh_tasks
from cluster_tools_amd.lifted_features import costs_from_node_labels as cost_tasks
from cluster_tools_amd.lifted_features import clear_lifted_edges_from_labels as clear_tasks


class LiftedFeaturesFromNodeLabelsWorkflow(WorkflowBase):
    ws_path = luigi.Parameter()
    ws_key = luigi.Parameter()
    labels_path = luigi.Parameter()
    labels_key = luigi.Parameter()
    graph_path = luigi.Parameter()
    graph_key = luigi.Parameter()
    output_path = luigi.Parameter()
    nh_out_key = luigi.Parameter()
    feat_out_key = luigi.Parameter()
    prefix = luigi.Parameter()
    nh_graph_depth = luigi.IntParameter(default=4)
    ignore_label = luigi.IntParameter(default=0)
    label_ignore_label = luigi.Parameter(default=None)
    label_overlap_threshold = luigi.FloatParameter(default=None)
    clear_labels_path = luigi.Parameter(default=None)
    clear_labels_key = luigi.Parameter(default=None)
    mode = luigi.Parameter(default='all')

    def _common(self, dep):
        return dict(tmp_folder=self.tmp_folder, config_dir=self.config_dir, max_jobs=self.max_jobs, dependency=dep)

    def _clear_lifted_edges(self, dep):
        # the fragments' labels under the clear labels (no ignore label there), then the lifted
        # edges between two of its objects go
        labels_key = 'node_overlaps/clear_%s' % self.prefix
        dep = NodeLabelWorkflow(target=self.target, ws_path=self.ws_path, ws_key=self.ws_key,
                                input_path=self.clear_labels_path, input_key=self.clear_labels_key,
                                prefix='clear_%s' % self.prefix, output_path=self.output_path,
                                output_key=labels_key, max_overlap=True, ignore_label=None, **self._common(dep))
        clear_task = getattr(clear_tasks, self._get_task_name('ClearLiftedEdgesFromLabels'))
        return clear_task(node_labels_path=self.output_path, node_labels_key=labels_key,
                          lifted_edge_path=self.output_path, lifted_edge_key=self.nh_out_key, **self._common(dep))

    def _node_labels(self, labels_key, dep):
        return NodeLabelWorkflow(target=self.target, ws_path=self.ws_path, ws_key=self.ws_key,
                                 input_path=self.labels_path, input_key=self.labels_key, prefix=self.prefix,
                                 output_path=self.output_path, output_key=labels_key, max_overlap=True,
                                 serialize_counts=False, ignore_label=self.label_ignore_label, **self._common(dep))

    def requires(self):
        if self.label_overlap_threshold is not None:
            raise NotImplementedError("lifted features: label_overlap_threshold=%r needs every node's overlap "
                                      "counts (NodeLabelWorkflow with serialize_counts, which it refuses for its "
                                      "1-D output); leave it None to label a node by its largest overlap"
                                      % (self.label_overlap_threshold,))
        # 1.) the fragments' labels under the segmentation in labels_path
        labels_key = 'node_overlaps/%s' % self.prefix
        dep = self._node_labels(labels_key, self.dependency)
        # 2.) the sparse lifted neighbourhood of the labelled nodes
        nh_task = getattr(nh_tasks, self._get_task_name('SparseLiftedNeighborhood'))
        dep = nh_task(graph_path=self.graph_path, graph_key=self.graph_key, node_label_path=self.output_path,
                      node_label_key=labels_key, output_path=self.output_path, output_key=self.nh_out_key,
                      nh_graph_depth=self.nh_graph_depth, mode=self.mode, prefix=self.prefix,
                      node_ignore_label=self.ignore_label, **self._common(dep))
        # with clear labels: only lifted edges inside one of their objects stay
        if self.clear_labels_path is not None:
            assert self.clear_labels_key is not None
            dep = self._clear_lifted_edges(dep)
        # 3.) the costs of the lifted edges
        cost_task = getattr(cost_tasks, self._get_task_name('CostsFromNodeLabels'))
        return cost_task(nh_path=self.output_path, nh_key=self.nh_out_key, node_label_path=self.output_path,
                         node_label_key=labels_key, output_path=self.output_path, output_key=self.feat_out_key,
                         prefix=self.prefix, **self._common(dep))

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({**NodeLabelWorkflow.get_config(),
                        'sparse_lifted_neighborhood': nh_tasks.SparseLiftedNeighborhoodLocal.default_task_config(),
                        'features_from_node_labels': cost_tasks.CostsFromNodeLabelsLocal.default_task_config(),
                        'clear_lifted_edges_from_labels':
                        clear_tasks.ClearLiftedEdgesFromLabelsLocal.default_task_config()})
        return configs
