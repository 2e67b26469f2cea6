#! /usr/bin/env python
"""InitialSubGraphs: the region adjacency graph of every block's extended box on the GPU
(cluster_tools/graph/initial_sub_graphs.py:21-153; task surface, config keys, `f.attrs['shape']`,
block list / retry handling and log lines unchanged).  The job replaces the loop over
`ndist.computeMergeableRegionGraph(..., increaseRoi=True)` (:106-120): one library handle per job,
blocks read ahead on a thread, the box [block.begin, min(block.end + 1, shape)) through
`Handle.rag_block`, the group `s0/sub_graphs/block_<id>` written per block."""
import os

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class InitialSubGraphsBase(luigi.Task):
    task_name = 'initial_sub_graphs'
    src_file = os.path.abspath(__file__)

    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    graph_path = luigi.Parameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'ignore_label': True})
        return config

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'graph_path': self.graph_path, 'block_shape': block_shape})
        # make the graph file and write the shape as attribute
        shape = vu.get_shape(self.input_path, self.input_key)
        with vu.file_reader(self.graph_path) as f:
            f.attrs['shape'] = list(shape)
        if self.n_retries == 0:
            block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        else:
            block_list = self.block_list
            self.clean_up_for_retry(block_list)
        n_jobs = min(len(block_list), self.max_jobs)
        self.prepare_jobs(n_jobs, block_list, config)
        self.submit_jobs(n_jobs)
        self.wait_for_jobs()
        self.check_jobs(n_jobs)


class InitialSubGraphsLocal(InitialSubGraphsBase, LocalTask):
    pass


class InitialSubGraphsSlurm(InitialSubGraphsBase, SlurmTask):
    pass


class InitialSubGraphsLSF(InitialSubGraphsBase, LSFTask):
    pass


#
# Implementation
#

def extended_bb(block, shape):
    """increaseRoi=True: the one-voxel upper halo, so every edge across a block face lands in the
    lower block's sub-graph."""
    return tuple(slice(b, min(e + 1, s)) for b, e, s in zip(block.begin, block.end, shape))


def run_graph_blocks(blocking, block_list, ds, f_graph, ignore_label):
    """`_graph_block` for every block of the job (initial_sub_graphs.py:106-120)."""
    from cluster_tools_amd import ctws
    from cluster_tools_amd.graph.serialization import write_graph
    shape = tuple(ds.shape)

    def read(block_id):
        bb = extended_bb(blocking.getBlock(block_id), shape)
        return bb, ds[bb]

    with ctws.Handle(fu.device()) as h, fu.read_ahead(read, block_list) as ahead:
        for block_id, nxt in ahead:
            fu.log("start processing block %i" % block_id)
            bb, labels = nxt.result()
            nodes, edges, _ = h.rag_block(labels, ignore_label)
            write_graph(f_graph, 's0/sub_graphs/block_%i' % block_id, nodes, edges, ignore_label,
                        roiBegin=[int(s.start) for s in bb], roiEnd=[int(s.stop) for s in bb])
            fu.log_block_success(block_id)


def initial_sub_graphs(job_id, config_path):
    config = fu.load_config(job_id, config_path)
    ignore_label = config.get('ignore_label', True)
    with vu.file_reader(config['input_path'], 'r') as f, vu.file_reader(config['graph_path']) as f_graph:
        ds = f[config['input_key']]
        blocking = Blocking([0, 0, 0], list(ds.shape), list(config['block_shape']))
        run_graph_blocks(blocking, config['block_list'], ds, f_graph, ignore_label)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(initial_sub_graphs)
