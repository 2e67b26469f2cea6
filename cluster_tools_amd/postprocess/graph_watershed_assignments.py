#! /usr/bin/env python
"""GraphWatershedAssignments: merge every segment listed in `discard_ids.npy` into a neighbour
along the cheapest graph edges (cluster_tools/postprocess/graph_watershed_assignments.py:21-186;
task surface, job config keys, the single job and log lines unchanged).  The job builds the seeds on
the host as the reference does (0 -> max + 1, discarded segments -> 0), replaces
`nifty.graph.edgeWeightedWatershedsSegmentation` (:172) by `Handle.graph_watershed`, maps the
offset back to 0 and, with `relabel`, renumbers by first appearance (vigra's `relabelConsecutive`,
start_label=1, keep_zeros).  With `from_costs` the weights are 1 - (c - min) / max(c - min) in the
reference's in-place numpy arithmetic, in the features' dtype: its rounding creates the ties the
flood then breaks by edge index.  The output is a uint64 dataset with the input's chunks, gzip.
Decided here (nifty is not available): DESIGN.md section 3.13."""
import os

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask
from cluster_tools_amd.postprocess.graph_connected_components import write_assignments


class GraphWatershedAssignmentsBase(luigi.Task):
    task_name = 'graph_watershed_assignments'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    problem_path = luigi.Parameter()
    graph_key = luigi.Parameter()
    features_key = luigi.Parameter()
    filter_nodes_path = luigi.Parameter()
    assignment_path = luigi.Parameter()
    assignment_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    relabel = luigi.BoolParameter(default=False)
    from_costs = luigi.BoolParameter(default=True)
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        config.update({'assignment_path': self.assignment_path, 'assignment_key': self.assignment_key,
                       'problem_path': self.problem_path, 'graph_key': self.graph_key,
                       'features_key': self.features_key, 'filter_nodes_path': self.filter_nodes_path,
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'from_costs': self.from_costs, 'relabel': self.relabel})
        n_jobs = 1
        self.prepare_jobs(n_jobs, None, config)
        self.submit_jobs(n_jobs)
        self.wait_for_jobs()
        self.check_jobs(n_jobs)


class GraphWatershedAssignmentsLocal(GraphWatershedAssignmentsBase, LocalTask):
    pass


class GraphWatershedAssignmentsSlurm(GraphWatershedAssignmentsBase, SlurmTask):
    pass


class GraphWatershedAssignmentsLSF(GraphWatershedAssignmentsBase, LSFTask):
    pass


#
# Implementation
#

def costs_to_weights(features):
    """Costs to weights in [0, 1], the largest cost at weight 0: the reference's three in-place
    steps in the features' own dtype (:137-141); -> a new array.  Equal costs divide 0 by 0: the
    NaN weights are then refused by the library."""
    features = np.array(features)
    features -= features.min()
    features /= features.max()
    return 1. - features


def relabel_first_appearance(labels):
    """vigra.analysis.relabelConsecutive(labels, start_label=1, keep_zeros=True): every non-zero
    label becomes 1 + the number of distinct non-zero labels that appear before its first entry."""
    labels = np.asarray(labels, dtype='uint64')
    values, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    number = np.zeros(len(values), dtype='uint64')
    nonzero = values != 0
    number[np.nonzero(nonzero)[0][np.argsort(first[nonzero], kind='stable')]] = np.arange(
        1, int(nonzero.sum()) + 1, dtype='uint64')
    return number[inverse.reshape(labels.shape)]


def load_problem(config):
    """What the flood reads, with the reference's checks, before any GPU call:
    -> (edges, weights, seeds, seed_offset, chunks of the assignment dataset)."""
    from cluster_tools_amd.graph.serialization import read_graph
    problem_path = config['problem_path']
    fu.log("Read features and edges from %s" % problem_path)
    with vu.file_reader(problem_path, 'r') as f:
        _, uv_ids = read_graph(f, config['graph_key'])
        ds = f[config['features_key']]
        features = ds[:, 0].squeeze() if ds.ndim == 2 else ds[:]
    assert len(features) == len(uv_ids), "%i features for %i edges" % (len(features), len(uv_ids))
    if config['from_costs'] and len(features):
        fu.log("Mapping costs with range %f to %f to range 0 to 1" % (features.min(), features.max()))
        features = costs_to_weights(features)
    assignment_path = config['assignment_path']
    fu.log("Read assignments from %s" % assignment_path)
    with vu.file_reader(assignment_path, 'r') as f:
        ds = f[config['assignment_key']]
        chunks = ds.chunks
        assignments = np.array(ds[:], dtype='uint64')
    assert assignments.ndim == 1, "the assignments are a node labelling, not a table of shape %s" % (assignments.shape,)
    n_nodes = int(uv_ids.max()) + 1 if len(uv_ids) else len(assignments)
    assert n_nodes == len(assignments),\
        "Expected number of nodes %i and number of assignments %i does not agree" % (n_nodes, len(assignments))
    seed_offset = int(assignments.max()) + 1

    discard_ids = np.load(config['filter_nodes_path'])
    assert 0 not in discard_ids, "Breaks logic"

    # map zero label to new id, discarded segments to 0
    assignments[assignments == 0] = seed_offset
    discard_mask = np.isin(assignments, discard_ids)
    assignments[discard_mask] = 0
    fu.log("Discarding %i fragments" % int(discard_mask.sum()))
    return uv_ids, features, assignments, seed_offset, chunks


def graph_watershed_assignments(job_id, config_path):
    from cluster_tools_amd import ctws
    config = fu.load_config(job_id, config_path)
    uv_ids, features, assignments, seed_offset, chunks = load_problem(config)
    fu.log("Start grah watershed")
    with ctws.Handle(fu.device()) as handle:
        assignments = handle.graph_watershed(uv_ids, features, assignments)
    fu.log("Finished graph watershed")
    assignments[assignments == seed_offset] = 0
    if config['relabel']:
        assignments = relabel_first_appearance(assignments)
    write_assignments(config['output_path'], config['output_key'], assignments, chunks)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(graph_watershed_assignments)
