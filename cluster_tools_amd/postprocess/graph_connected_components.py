#! /usr/bin/env python
"""GraphConnectedComponents: split the segments of a fragment-segment assignment that are not
connected in the fragment graph (cluster_tools/postprocess/graph_connected_components.py:19-123;
task surface, job config keys, the single job and log lines unchanged).  The job replaces
`ndist.connectedComponentsFromNodes(graph, assignments, True)` and vigra's `relabelConsecutive`
(:110-114) by `Handle.graph_components`: the graph's `edges` table and the assignments go to the
GPU, and the components come back numbered from 1 in the order of their smallest fragment id, with
0 kept for fragments assigned to 0.  The output is a uint64 dataset with the input's chunks, gzip.
Decided here (nifty is not available): DESIGN.md section 3.13."""
import os

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class GraphConnectedComponentsBase(luigi.Task):
    task_name = 'graph_connected_components'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    problem_path = luigi.Parameter()
    graph_key = luigi.Parameter()
    assignment_path = luigi.Parameter()
    assignment_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        config.update({'problem_path': self.problem_path, 'graph_key': self.graph_key,
                       'assignment_path': self.assignment_path, 'assignment_key': self.assignment_key,
                       'output_key': self.output_key, 'output_path': self.output_path})
        n_jobs = 1
        self.prepare_jobs(n_jobs, None, config)
        self.submit_jobs(n_jobs)
        self.wait_for_jobs()
        self.check_jobs(n_jobs)


class GraphConnectedComponentsLocal(GraphConnectedComponentsBase, LocalTask):
    pass


class GraphConnectedComponentsSlurm(GraphConnectedComponentsBase, SlurmTask):
    pass


class GraphConnectedComponentsLSF(GraphConnectedComponentsBase, LSFTask):
    pass


#
# Implementation
#

def write_assignments(path, key, assignments, chunks):
    """The node labelling as the uint64 dataset `key` with the input's chunks, gzip."""
    with vu.file_reader(path) as f:
        ds = f.require_dataset(key, shape=assignments.shape, chunks=tuple(chunks), compression='gzip', dtype='uint64')
        ds[:] = np.ascontiguousarray(assignments, dtype='uint64')


def graph_connected_components(job_id, config_path):
    from cluster_tools_amd import ctws
    from cluster_tools_amd.graph.serialization import read_graph
    config = fu.load_config(job_id, config_path)
    with vu.file_reader(config['assignment_path'], 'r') as f:
        ds_ass = f[config['assignment_key']]
        assignments = ds_ass[:]
        chunks = ds_ass.chunks
    assert assignments.ndim == 1, "the assignments are a node labelling, not a table of shape %s" % (assignments.shape,)
    with vu.file_reader(config['problem_path'], 'r') as f:
        _, edges = read_graph(f, config['graph_key'])
    with ctws.Handle(fu.device()) as handle:
        assignments = handle.graph_components(edges, assignments)
    write_assignments(config['output_path'], config['output_key'], assignments, chunks)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(graph_connected_components)
