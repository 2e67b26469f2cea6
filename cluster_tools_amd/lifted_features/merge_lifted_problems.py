#! /usr/bin/env python
"""MergeLiftedProblems: several lifted problems of one file into one
(cluster_tools/lifted_features/merge_lifted_problems.py:19-141; task surface, job config keys, the
one job under `out_prefix` and the dataset names s0/lifted_nh_<prefix>, s0/lifted_costs_<prefix>
unchanged).  The edges and costs of the problems are concatenated in the order of `prefixs`.  As in
the reference (:121-125), the rows are NOT sorted again and an edge that two problems share stays
twice, each time with its own cost: a solver that wants it once sums them.  Chunks of
min(k, 100000) rows.  `prefixs` is a list (the reference declares an IntParameter and hands it a
list).  Id tables: numpy on the host."""
import os

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask

EDGE_ROOT = 's0/lifted_nh_%s'
COST_ROOT = 's0/lifted_costs_%s'


class MergeLiftedProblemsBase(luigi.Task):
    task_name = 'merge_lifted_problems'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    path = luigi.Parameter()
    prefixs = luigi.ListParameter()
    out_prefix = luigi.Parameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        config.update({'path': self.path, 'prefixs': list(self.prefixs), 'out_prefix': self.out_prefix})
        self.prepare_jobs(1, None, config, self.out_prefix)
        self.submit_jobs(1, self.out_prefix)
        self.wait_for_jobs(self.out_prefix)
        self.check_jobs(1, self.out_prefix)

    def output(self):
        return luigi.LocalTarget(os.path.join(self.tmp_folder, self.task_name + '_%s.log' % self.out_prefix))


class MergeLiftedProblemsLocal(MergeLiftedProblemsBase, LocalTask):
    pass


class MergeLiftedProblemsSlurm(MergeLiftedProblemsBase, SlurmTask):
    pass


class MergeLiftedProblemsLSF(MergeLiftedProblemsBase, LSFTask):
    pass


#
# Implementation
#

def merge_lifted_problems(job_id, config_path):
    config = fu.load_config(job_id, config_path)
    out_prefix = config['out_prefix']
    with vu.file_reader(config['path']) as f:
        edges, costs = [], []
        for prefix in config['prefixs']:
            this_edges = f[EDGE_ROOT % prefix][:]
            this_costs = f[COST_ROOT % prefix][:]
            assert len(this_costs) == len(this_edges), "problem %s: %i costs for %i lifted edges" % (
                prefix, len(this_costs), len(this_edges))
            edges.append(this_edges)
            costs.append(this_costs)
        edges = np.concatenate(edges, axis=0)
        costs = np.concatenate(costs, axis=0)
        ds = f.require_dataset(EDGE_ROOT % out_prefix, shape=edges.shape, compression='gzip', dtype=edges.dtype,
                               chunks=(min(len(edges), 100000), 2))
        ds[:] = edges
        ds = f.require_dataset(COST_ROOT % out_prefix, shape=costs.shape, compression='gzip', dtype=costs.dtype,
                               chunks=(min(len(costs), 100000),))
        ds[:] = costs
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(merge_lifted_problems)
