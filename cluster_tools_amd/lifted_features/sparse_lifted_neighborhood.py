#! /usr/bin/env python
"""SparseLiftedNeighborhood: the lifted edges of the graph under a node labelling
(cluster_tools/lifted_features/sparse_lifted_neighborhood.py:19-139; task surface, job config keys,
the one job under `prefix` and log lines unchanged).  The job replaces
`ndist.computeLiftedNeighborhoodFromNodeLabels` (:132-135) by `Handle.lifted_neighborhood`: the
graph's `edges` table and the node labels go to the GPU, the pairs of labelled nodes 2 .. depth hops
apart that pass the mode test come back sorted and are written as (k, 2) uint64, gzip, chunks
(min(k, 262144), 2).  A graph without a lifted edge has no dataset to write (an n5 dataset has no
zero extent, and the reference cannot represent it either): the job raises and writes nothing.
Decided here (nifty is not available): DESIGN.md section 3.12."""
import os

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask

CHUNK = 262144  # rows per chunk


class SparseLiftedNeighborhoodBase(luigi.Task):
    task_name = 'sparse_lifted_neighborhood'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    graph_path = luigi.Parameter()
    graph_key = luigi.Parameter()
    node_label_path = luigi.Parameter()
    node_label_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    prefix = luigi.Parameter()
    nh_graph_depth = luigi.IntParameter()
    node_ignore_label = luigi.IntParameter(default=0)
    # 'all': lifted edges between all labelled nodes, 'same': only between nodes of one label,
    # 'different': only between nodes of different labels
    mode = luigi.Parameter(default='all')
    dependency = luigi.TaskParameter()

    modes = ('all', 'same', 'different')

    def requires(self):
        return self.dependency

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        assert self.mode in self.modes, "Invalid mode %s" % self.mode
        config = self.get_task_config()
        config.update({'graph_path': self.graph_path, 'graph_key': self.graph_key,
                       'node_label_path': self.node_label_path, 'node_label_key': self.node_label_key,
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'nh_graph_depth': self.nh_graph_depth, 'node_ignore_label': self.node_ignore_label,
                       'mode': self.mode})
        self.prepare_jobs(1, None, config, self.prefix)
        self.submit_jobs(1, self.prefix)
        self.wait_for_jobs(self.prefix)
        self.check_jobs(1, self.prefix)

    def output(self):
        return luigi.LocalTarget(os.path.join(self.tmp_folder, self.task_name + '_%s.log' % self.prefix))


class SparseLiftedNeighborhoodLocal(SparseLiftedNeighborhoodBase, LocalTask):
    pass


class SparseLiftedNeighborhoodSlurm(SparseLiftedNeighborhoodBase, SlurmTask):
    pass


class SparseLiftedNeighborhoodLSF(SparseLiftedNeighborhoodBase, LSFTask):
    pass


#
# Implementation
#

def write_lifted_edges(f, key, lifted):
    """The lifted edges as the dataset `key` of f; a table left by an earlier run is replaced."""
    lifted = np.ascontiguousarray(lifted, dtype='uint64').reshape(-1, 2)
    k = len(lifted)
    assert k, "an n5 dataset has no zero extent"
    if key in f:
        del f[key]
    return f.create_dataset(key, data=lifted, chunks=(min(k, CHUNK), 2), compression='gzip')


def sparse_lifted_neighborhood(job_id, config_path):
    from cluster_tools_amd import ctws
    from cluster_tools_amd.graph.serialization import read_table
    config = fu.load_config(job_id, config_path)
    graph_depth = config['nh_graph_depth']
    node_ignore_label = config['node_ignore_label']
    mode = config.get('mode', 'all')
    fu.log("lifted nh mode set to %s, depth set to %i" % (mode, graph_depth))
    fu.log("have ignore label: %i" % node_ignore_label)
    with vu.file_reader(config['graph_path'], 'r') as f:
        edges = read_table(f[config['graph_key']], 'edges', 2)
    with vu.file_reader(config['node_label_path'], 'r') as f:
        node_labels = f[config['node_label_key']][:]
    fu.log("start lifted neighborhood extraction for depth %i" % graph_depth)
    with ctws.Handle(fu.device()) as handle:
        lifted = handle.lifted_neighborhood(edges, node_labels, graph_depth, mode, node_ignore_label)
    if len(lifted) == 0:
        raise RuntimeError("sparse_lifted_neighborhood: no lifted edge for depth %i and mode %s (%i graph edges, "
                           "%i labelled nodes): there is nothing to write"
                           % (graph_depth, mode, len(edges),
                              int((node_labels != np.uint64(node_ignore_label & 0xFFFFFFFFFFFFFFFF)).sum())))
    with vu.file_reader(config['output_path']) as f:
        write_lifted_edges(f, config['output_key'], lifted)
    with vu.file_reader(config['output_path'], 'r') as f:
        n_lifted = f[config['output_key']].shape[0]
    fu.log("extracted %i lifted edges" % n_lifted)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(sparse_lifted_neighborhood)
