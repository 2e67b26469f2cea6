#! /usr/bin/env python
"""CostsFromNodeLabels: a cost per lifted edge from the two node labels
(cluster_tools/lifted_features/costs_from_node_labels.py:21-177; task surface, config keys
intra_label_cost / inter_label_cost, job config keys, the split of the edge chunks of
min(262144, k) rows over the jobs and log lines unchanged).  Per lifted edge, float32:
intra_label_cost (6 by default, attractive) when the two labels are equal, inter_label_cost (-6,
repulsive) otherwise; an endpoint with label 0 is an error, as the reference's assert (:131).
These are id tables, not voxels: the job runs on the host with numpy, as MergeEdgeFeatures does."""
import os

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class CostsFromNodeLabelsBase(luigi.Task):
    task_name = 'costs_from_node_labels'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    nh_path = luigi.Parameter()
    nh_key = luigi.Parameter()
    node_label_path = luigi.Parameter()
    node_label_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    prefix = luigi.Parameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        # intra_label_cost: a lifted edge between two nodes of one label (very attractive: 6 is
        # close to the usual largest cost); inter_label_cost: between different labels (very repulsive)
        config.update({'intra_label_cost': 6., 'inter_label_cost': -6.})
        return config

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        with vu.file_reader(self.nh_path, 'r') as f:
            n_lifted_edges = int(f[self.nh_key].shape[0])
        chunk_size = min(262144, n_lifted_edges)
        with vu.file_reader(self.output_path) as f:
            f.require_dataset(self.output_key, shape=(n_lifted_edges,), chunks=(chunk_size,), compression='gzip',
                              dtype='float32')
        config.update({'nh_path': self.nh_path, 'nh_key': self.nh_key,
                       'node_label_path': self.node_label_path, 'node_label_key': self.node_label_key,
                       'output_path': self.output_path, 'output_key': self.output_key, 'chunk_size': chunk_size})
        edge_block_list = vu.blocks_in_volume([n_lifted_edges], [chunk_size])
        n_jobs = min(self.max_jobs, len(edge_block_list))
        self.prepare_jobs(n_jobs, edge_block_list, config, self.prefix)
        self.submit_jobs(n_jobs, self.prefix)
        self.wait_for_jobs(self.prefix)
        self.check_jobs(n_jobs, self.prefix)

    def output(self):
        return luigi.LocalTarget(os.path.join(self.tmp_folder, self.task_name + '_%s.log' % self.prefix))


class CostsFromNodeLabelsLocal(CostsFromNodeLabelsBase, LocalTask):
    pass


class CostsFromNodeLabelsSlurm(CostsFromNodeLabelsBase, SlurmTask):
    pass


class CostsFromNodeLabelsLSF(CostsFromNodeLabelsBase, LSFTask):
    pass


#
# Implementation
#

def costs_for_edges(uv_ids, node_labels, intra_label_cost, inter_label_cost):
    """float32 (k,): the cost of every lifted edge (k, 2) under the node labels."""
    uv_ids = np.asarray(uv_ids).reshape(-1, 2).astype('int64')
    labels_a = node_labels[uv_ids[:, 0]]
    labels_b = node_labels[uv_ids[:, 1]]
    n_unlabelled = int((labels_a == 0).sum() + (labels_b == 0).sum())
    if n_unlabelled:
        raise ValueError("costs_from_node_labels: %i endpoints of lifted edges have the node label 0; the lifted "
                         "neighbourhood joins labelled nodes only" % n_unlabelled)
    edge_costs = np.full(len(uv_ids), intra_label_cost, dtype='float32')
    edge_costs[labels_a != labels_b] = inter_label_cost
    return edge_costs


def _costs_for_edge_block(block_id, blocking, ds_in, ds_out, node_labels, inter_label_cost, intra_label_cost):
    fu.log("start processing block %i" % block_id)
    block = blocking.getBlock(block_id)
    id_begin, id_end = int(block.begin[0]), int(block.end[0])
    ds_out[id_begin:id_end] = costs_for_edges(ds_in[id_begin:id_end], node_labels, intra_label_cost,
                                              inter_label_cost)
    fu.log_block_success(block_id)


def costs_from_node_labels(job_id, config_path):
    config = fu.load_config(job_id, config_path)
    chunk_size = config['chunk_size']
    inter_label_cost, intra_label_cost = config['inter_label_cost'], config['intra_label_cost']
    with vu.file_reader(config['node_label_path'], 'r') as f:
        node_labels = f[config['node_label_key']][:]
    with vu.file_reader(config['nh_path']) as f_in, vu.file_reader(config['output_path']) as f_out:
        ds_in = f_in[config['nh_key']]
        ds_out = f_out[config['output_key']]
        n_lifted_edges = int(ds_in.shape[0])
        blocking = Blocking([0], [n_lifted_edges], [chunk_size])
        for block_id in config['block_list']:
            _costs_for_edge_block(block_id, blocking, ds_in, ds_out, node_labels, inter_label_cost,
                                  intra_label_cost)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(costs_from_node_labels)
