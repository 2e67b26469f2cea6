#! /usr/bin/env python
"""BlockEdgeFeatures: the boundary-map statistics of every block's edges on the GPU
(cluster_tools/features/block_edge_features.py:18-320; task surface, config keys, job config keys
and log lines unchanged).  The job replaces `ndist.extractBlockFeaturesFromBoundaryMaps_*`
(:113-132): one library handle per job, blocks read ahead on a thread, labels and boundary map on
the box [block.begin, min(block.end + 1, shape)) through `Handle.edge_features_block` with the
sub-graph `s0/sub_graphs/block_<id>`, the table `blocks/block_<id>` (m, 10) written per block.
The filter-response path (`filters`, `sigmas`) and the affinity path (`offsets`) are not built:
a config that sets one of them is refused before any block is processed."""
import os

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class BlockEdgeFeaturesBase(luigi.Task):
    task_name = 'block_edge_features'
    src_file = os.path.abspath(__file__)

    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    labels_path = luigi.Parameter()
    labels_key = luigi.Parameter()
    graph_path = luigi.Parameter()
    output_path = luigi.Parameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'offsets': None, 'filters': None, 'sigmas': None, 'halo': [0, 0, 0],
                       'apply_in_2d': False, 'channel_agglomeration': 'mean'})
        return config

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        check_supported(config)
        with vu.file_reader(self.output_path) as f:
            f.require_group('blocks')
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'labels_path': self.labels_path, 'labels_key': self.labels_key,
                       'output_path': self.output_path, 'block_shape': block_shape,
                       'graph_block_prefix': os.path.join(self.graph_path, 's0', 'sub_graphs', 'block_')})
        if self.n_retries == 0:
            shape = vu.get_shape(self.input_path, self.input_key)
            if len(shape) == 4:
                shape = shape[1:]
            block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        else:
            block_list = self.block_list
            self.clean_up_for_retry(block_list)
        n_jobs = min(len(block_list), self.max_jobs)
        self.prepare_jobs(n_jobs, block_list, config)
        self.submit_jobs(n_jobs)
        self.wait_for_jobs()
        self.check_jobs(n_jobs)


class BlockEdgeFeaturesLocal(BlockEdgeFeaturesBase, LocalTask):
    pass


class BlockEdgeFeaturesSlurm(BlockEdgeFeaturesBase, SlurmTask):
    pass


class BlockEdgeFeaturesLSF(BlockEdgeFeaturesBase, LSFTask):
    pass


#
# Implementation
#

def check_supported(config):
    """Only the plain boundary-map accumulation runs here (block_edge_features.py:113-132)."""
    for key, what in (('filters', 'filter responses (vu.apply_filter + ndist.accumulateInput)'),
                      ('sigmas', 'filter responses (vu.apply_filter + ndist.accumulateInput)'),
                      ('offsets', 'affinity maps (ndist.extractBlockFeaturesFromAffinityMaps_*)')):
        if config.get(key) is not None:
            raise NotImplementedError("block_edge_features: '%s' is set, but edge features from %s are not "
                                      "implemented on the GPU; only 3-D boundary maps are" % (key, what))


def run_feature_blocks(blocking, block_list, ds_in, ds_labels, f_graph, f_out):
    """The boundary-map accumulation for every block of the job."""
    from cluster_tools_amd import ctws
    from cluster_tools_amd.graph.serialization import read_table
    from cluster_tools_amd.graph.initial_sub_graphs import extended_bb
    shape = tuple(ds_labels.shape)

    def read(block_id):
        g = f_graph['s0/sub_graphs/block_%i' % block_id]
        edges = read_table(g, 'edges', 2)
        if len(edges) == 0:
            return None
        block = blocking.getBlock(block_id)
        bb = extended_bb(block, shape)
        core = [int(e - b) for b, e in zip(block.begin, block.end)]
        return read_table(g, 'nodes'), edges, bool(g.attrs['ignoreLabel']), core, ds_labels[bb], ds_in[bb]

    with ctws.Handle(fu.device()) as h, fu.read_ahead(read, block_list) as ahead:
        for block_id, nxt in ahead:
            fu.log("start processing block %i" % block_id)
            item = nxt.result()
            if item is None:
                fu.log("block %i has no edges" % block_id)
                fu.log_block_success(block_id)
                continue
            nodes, edges, ignore_label, core, labels, data = item
            feats, n_missing = h.edge_features_block(labels, data, nodes, edges, ignore_label, core)
            if n_missing > 0:
                raise RuntimeError("block %i: %i voxel pairs have an edge that is not in the block's sub-graph"
                                   % (block_id, n_missing))
            key = 'blocks/block_%i' % block_id
            fu.log("saving feature result of shape %s to %s" % (str(feats.shape), os.path.join(f_out.path, key)))
            if key in f_out:  # a retried block
                del f_out[key]
            f_out.create_dataset(key, data=feats, chunks=feats.shape)
            fu.log_block_success(block_id)


def block_edge_features(job_id, config_path):
    config = fu.load_config(job_id, config_path)
    check_supported(config)
    graph_path = os.path.normpath(os.path.join(config['graph_block_prefix'], '..', '..', '..'))
    fu.log("accumulate features without applying filters")
    with vu.file_reader(config['input_path'], 'r') as f, vu.file_reader(config['labels_path'], 'r') as f_l, \
            vu.file_reader(graph_path, 'r') as f_graph, vu.file_reader(config['output_path']) as f_out:
        ds_in, ds_labels = f[config['input_key']], f_l[config['labels_key']]
        if ds_in.ndim != 3:
            raise NotImplementedError("block_edge_features: the boundary map must be 3-D, not %i-D" % ds_in.ndim)
        if str(ds_in.dtype) not in ('float32', 'uint8'):
            raise TypeError("block_edge_features: the boundary map must be float32 or uint8, not %s" % ds_in.dtype)
        assert tuple(ds_in.shape) == tuple(ds_labels.shape), (ds_in.shape, ds_labels.shape)
        fu.log('accumulate boundary map for type %s' % str(ds_in.dtype))
        blocking = Blocking([0, 0, 0], list(ds_labels.shape), list(config['block_shape']))
        run_feature_blocks(blocking, config['block_list'], ds_in, ds_labels, f_graph, f_out)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(block_edge_features)
