#! /usr/bin/env python
"""ClearLiftedEdgesFromLabels: drop the lifted edges that join two objects of a second labelling
(cluster_tools/lifted_features/clear_lifted_edges_from_labels.py:19-128; task surface, job config
keys, the one job without a prefix and log lines unchanged).  A lifted edge stays iff its two
endpoints have equal labels in `node_labels`; the dataset is written again, with its chunks, only
when rows were dropped.  If none stays there is nothing an n5 dataset could hold: the job raises
and leaves the dataset as it was.  An id table: numpy on the host."""
import os

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class ClearLiftedEdgesFromLabelsBase(luigi.Task):
    task_name = 'clear_lifted_edges_from_labels'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    node_labels_path = luigi.Parameter()
    node_labels_key = luigi.Parameter()
    lifted_edge_path = luigi.Parameter()
    lifted_edge_key = luigi.Parameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        config.update({'node_labels_path': self.node_labels_path, 'node_labels_key': self.node_labels_key,
                       'lifted_edge_path': self.lifted_edge_path, 'lifted_edge_key': self.lifted_edge_key})
        self.prepare_jobs(1, None, config)
        self.submit_jobs(1)
        self.wait_for_jobs()
        self.check_jobs(1)


class ClearLiftedEdgesFromLabelsLocal(ClearLiftedEdgesFromLabelsBase, LocalTask):
    pass


class ClearLiftedEdgesFromLabelsSlurm(ClearLiftedEdgesFromLabelsBase, SlurmTask):
    pass


class ClearLiftedEdgesFromLabelsLSF(ClearLiftedEdgesFromLabelsBase, LSFTask):
    pass


#
# Implementation
#

def clear_edges(lifted_edges, node_labels):
    """The rows of lifted_edges (k, 2) whose two endpoints have one label."""
    lifted_mapped = node_labels[lifted_edges.astype('int64')]
    return lifted_edges[lifted_mapped[:, 0] == lifted_mapped[:, 1]]


def clear_lifted_edges_from_labels(job_id, config_path):
    config = fu.load_config(job_id, config_path)
    lifted_edge_key = config['lifted_edge_key']
    with vu.file_reader(config['node_labels_path'], 'r') as f:
        node_labels = f[config['node_labels_key']][:]
    with vu.file_reader(config['lifted_edge_path']) as f:
        ds = f[lifted_edge_key]
        lifted_edges = ds[:]
        chunks = tuple(ds.chunks)
        n_lifted = len(lifted_edges)
        lifted_edges = clear_edges(lifted_edges, node_labels)
        n_lifted_new = len(lifted_edges)
        fu.log("clear number of lifted edges from %i to %i" % (n_lifted, n_lifted_new))
        if n_lifted_new == 0:
            raise RuntimeError("clear_lifted_edges_from_labels: none of the %i lifted edges joins two nodes of one "
                               "label: there is nothing to write" % n_lifted)
        # the dataset is written again iff rows were dropped
        if n_lifted_new < n_lifted:
            del f[lifted_edge_key]
            f.create_dataset(lifted_edge_key, data=lifted_edges, chunks=chunks, compression='gzip')
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(clear_lifted_edges_from_labels)
