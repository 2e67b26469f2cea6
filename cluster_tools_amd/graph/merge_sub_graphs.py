#! /usr/bin/env python
"""MergeSubGraphs: the union of sub-graphs, per block of a coarser scale or of all blocks into
the final graph (cluster_tools/graph/merge_sub_graphs.py:20-208; parameters, config keys and log
lines unchanged).  `ndist.mergeSubgraphs` (:133-158) becomes the GPU unique of the concatenated
children's nodes and `Handle.unique_pairs_u64` of their concatenated edges.

Not the reference's: its `_merge_subblocks` reads and writes `sub_graphs/s%i/block_` while every
other place uses `s%i/sub_graphs/block_` (n_scales > 1 cannot run as written); here it is
`s<scale>/sub_graphs/block_<id>` throughout.  The task that merges the blocks of a scale writes
the log `merge_sub_graphs_s<scale>_blocks.log`, the one that merges the complete graph
`merge_sub_graphs_s<scale>.log`: with one name for both, the two tasks GraphWorkflow runs at
scale n_scales - 1 would share their target."""
import os

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class MergeSubGraphsBase(luigi.Task):
    task_name = 'merge_sub_graphs'
    src_file = os.path.abspath(__file__)

    graph_path = luigi.Parameter()
    scale = luigi.IntParameter()
    output_key = luigi.Parameter(default='')
    merge_complete_graph = luigi.BoolParameter(default=False)
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        config.update({'graph_path': self.graph_path, 'block_shape': block_shape, 'scale': self.scale,
                       'merge_complete_graph': self.merge_complete_graph, 'output_key': self.output_key,
                       'roi_begin': roi_begin, 'roi_end': roi_end})
        with vu.file_reader(self.graph_path) as f:
            shape = f.attrs['shape']
        factor = 2 ** self.scale
        block_shape = tuple(sh * factor for sh in block_shape)
        if self.n_retries == 0:
            block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        else:
            block_list = self.block_list
            self.clean_up_for_retry(block_list)
        # the complete graph is merged by one job
        n_jobs = 1 if self.merge_complete_graph else min(len(block_list), self.max_jobs)
        self.prepare_jobs(n_jobs, block_list, config)
        self.submit_jobs(n_jobs)
        self.wait_for_jobs()
        self.check_jobs(n_jobs)

    def output(self):
        name = '_s%i.log' if self.merge_complete_graph else '_s%i_blocks.log'
        return luigi.LocalTarget(os.path.join(self.tmp_folder, self.task_name + name % self.scale))


class MergeSubGraphsLocal(MergeSubGraphsBase, LocalTask):
    pass


class MergeSubGraphsSlurm(MergeSubGraphsBase, SlurmTask):
    pass


class MergeSubGraphsLSF(MergeSubGraphsBase, LSFTask):
    pass


#
# Implementation
#

def merge_graphs(h, f, block_prefix, block_ids, output_key, **attrs):
    """The union of the groups block_prefix + id: sorted unique nodes, sorted unique edges."""
    from cluster_tools_amd.graph.serialization import read_graph, write_graph
    nodes, edges, ignore_label = [], [], True
    for i, block_id in enumerate(block_ids):
        key = block_prefix + str(block_id)
        n, e = read_graph(f, key)
        if i == 0:
            ignore_label = bool(f[key].attrs.get('ignoreLabel', True))
        nodes.append(n)
        edges.append(e)
    nodes = np.concatenate(nodes) if nodes else np.zeros(0, 'uint64')
    edges = np.concatenate(edges) if edges else np.zeros((0, 2), 'uint64')
    nodes = h.unique_u64(nodes) if len(nodes) else nodes
    edges = h.unique_pairs_u64(edges)[0] if len(edges) else edges
    return write_graph(f, output_key, nodes, edges, ignore_label, **attrs)


def merge_sub_graphs(job_id, config_path):
    from cluster_tools_amd import ctws
    config = fu.load_config(job_id, config_path)
    scale = config['scale']
    initial_block_shape = config['block_shape']
    block_list = config['block_list']
    with vu.file_reader(config['graph_path']) as f, ctws.Handle(fu.device()) as h:
        shape = list(f.attrs['shape'])
        if config['merge_complete_graph']:
            fu.log("merge complete graph at scale %i" % scale)
            output_key = config.get('output_key', '')
            assert output_key != ''
            merge_graphs(h, f, 's%i/sub_graphs/block_' % scale, block_list, output_key, shape=shape)
        else:
            fu.log("merging subgraphs at scale %i" % scale)
            blocking = Blocking([0, 0, 0], shape, [2 ** scale * bs for bs in initial_block_shape])
            previous_shape = [2 ** (scale - 1) * bs for bs in initial_block_shape]
            previous_blocking = Blocking([0, 0, 0], shape, previous_shape)
            # with a global roi only the children inside it have a sub-graph
            scheduled = set(vu.blocks_in_volume(shape, previous_shape, config.get('roi_begin'),
                                                config.get('roi_end')))
            for block_id in block_list:
                fu.log("start processing block %i" % block_id)
                block = blocking.getBlock(block_id)
                children = previous_blocking.getBlockIdsOverlappingBoundingBox(block.begin, block.end).tolist()
                children = [int(c) for c in children if int(c) in scheduled]
                merge_graphs(h, f, 's%i/sub_graphs/block_' % (scale - 1), children,
                             's%i/sub_graphs/block_%i' % (scale, block_id), roiBegin=[int(b) for b in block.begin],
                             roiEnd=[int(min(e + 1, s)) for e, s in zip(block.end, shape)])
                fu.log_block_success(block_id)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(merge_sub_graphs)
