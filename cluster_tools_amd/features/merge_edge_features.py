#! /usr/bin/env python
"""MergeEdgeFeatures: the blocks' feature tables into the table of the global graph's edges
(cluster_tools/features/merge_edge_features.py:19-174; task surface, config keys, job config keys,
the consecutive split of the edge chunks over the jobs and log lines unchanged).  The job replaces
`ndist.mergeFeatureBlocks` (:159-165).  These are id tables, not voxels: the merge runs on the
host with numpy over the blocks' `edgeIds`, as MapEdgeIds does.  Per global edge, over the rows
with that id and w = their count: count = sum w, mean and every quantile the w-weighted average,
variance = sum w (var + (mean_r - mean)^2) / count, min / max over the rows with w > 0.  An edge
without a row stays 0.  Restated (nifty is not available): DESIGN.md section 3.5."""
import os

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class MergeEdgeFeaturesBase(luigi.Task):
    task_name = 'merge_edge_features'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    graph_path = luigi.Parameter()
    graph_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def _read_num_features(self, block_ids):
        with vu.file_reader(self.output_path, 'r') as f:
            for block_id in block_ids:
                key = 'blocks/block_%i' % block_id
                if key in f:
                    return int(f[key].shape[1])
        raise AssertionError("No valid feature block found")

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        with vu.file_reader(self.graph_path, 'r') as f:
            shape = list(f.attrs['shape'])
            n_edges = int(f[self.graph_key].attrs['numberOfEdges'])
        # without a roi only the number of blocks is serialized, else the blocks in the roi
        if roi_begin is None:
            block_ids = Blocking([0, 0, 0], shape, list(block_shape)).numberOfBlocks
        else:
            block_ids = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        chunk_size = min(262144, n_edges)
        n_features = self._read_num_features(range(block_ids) if isinstance(block_ids, int) else block_ids)
        with vu.file_reader(self.output_path) as f:
            f.require_dataset(self.output_key, dtype='float64', shape=(n_edges, n_features),
                              chunks=(chunk_size, 1), compression='gzip')
        config.update({'graph_block_prefix': os.path.join(self.graph_path, 's0', 'sub_graphs', 'block_'),
                       'feature_block_prefix': os.path.join(self.output_path, 'blocks', 'block_'),
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'edge_chunk_size': chunk_size, 'block_ids': block_ids, 'n_edges': n_edges})
        edge_block_list = vu.blocks_in_volume([n_edges], [chunk_size])
        n_jobs = min(len(edge_block_list), self.max_jobs)
        self.prepare_jobs(n_jobs, edge_block_list, config, consecutive_blocks=True)
        self.submit_jobs(n_jobs)
        self.wait_for_jobs()
        self.check_jobs(n_jobs)


class MergeEdgeFeaturesLocal(MergeEdgeFeaturesBase, LocalTask):
    pass


class MergeEdgeFeaturesSlurm(MergeEdgeFeaturesBase, SlurmTask):
    pass


class MergeEdgeFeaturesLSF(MergeEdgeFeaturesBase, LSFTask):
    pass


#
# Implementation
#

def merge_feature_rows(ids, rows, edge_begin, edge_end):
    """The merged rows of the global edges [edge_begin, edge_end) from the blocks' rows (n, 10)
    with their global edge ids (n,); rows of other edges are ignored."""
    n_out = edge_end - edge_begin
    n_feats = rows.shape[1]
    out = np.zeros((n_out, n_feats), dtype='float64')
    sel = (ids >= edge_begin) & (ids < edge_end)
    ids, rows = (ids[sel] - edge_begin).astype('int64'), rows[sel]
    w = rows[:, -1]
    count = np.bincount(ids, weights=w, minlength=n_out)
    has = count > 0
    div = np.where(has, count, 1.)
    out[:, 0] = np.bincount(ids, weights=w * rows[:, 0], minlength=n_out) / div
    out[:, 1] = np.bincount(ids, weights=w * (rows[:, 1] + (rows[:, 0] - out[ids, 0]) ** 2), minlength=n_out) / div
    for col in range(3, n_feats - 2):
        out[:, col] = np.bincount(ids, weights=w * rows[:, col], minlength=n_out) / div
    pos = w > 0
    lo, hi = np.full(n_out, np.inf), np.full(n_out, -np.inf)
    np.minimum.at(lo, ids[pos], rows[pos, 2])
    np.maximum.at(hi, ids[pos], rows[pos, -2])
    out[:, 2], out[:, -2] = np.where(has, lo, 0.), np.where(has, hi, 0.)
    out[:, -1] = count
    return out


def merge_edge_features(job_id, config_path):
    from cluster_tools_amd.graph.serialization import read_table
    config = fu.load_config(job_id, config_path)
    edge_block_list = config['block_list']
    assert (np.diff(edge_block_list) == 1).all(), "the edge chunks of a job are consecutive"
    n_edges, chunk = config['n_edges'], config['edge_chunk_size']
    edge_blocking = Blocking([0], [n_edges], [chunk])
    edge_begin = int(edge_blocking.getBlock(edge_block_list[0]).begin[0])
    edge_end = int(edge_blocking.getBlock(edge_block_list[-1]).end[0])
    block_ids = config['block_ids']
    block_ids = list(range(block_ids)) if isinstance(block_ids, int) else block_ids
    graph_path = os.path.normpath(os.path.join(config['graph_block_prefix'], '..', '..', '..'))
    ids, rows = [], []
    with vu.file_reader(graph_path, 'r') as f_graph, vu.file_reader(config['output_path']) as f_out:
        for block_id in block_ids:
            key = 'blocks/block_%i' % block_id
            if key not in f_out:  # a block without edges
                continue
            feats = f_out[key][:]
            edge_ids = read_table(f_graph['s0/sub_graphs/block_%i' % block_id], 'edgeIds')
            assert len(edge_ids) == len(feats), "block %i: %i edge ids, %i feature rows" % (block_id, len(edge_ids),
                                                                                            len(feats))
            ids.append(edge_ids.astype('int64'))
            rows.append(feats)
        ds = f_out[config['output_key']]
        n_feats = int(ds.shape[1])
        ids = np.concatenate(ids) if ids else np.zeros(0, 'int64')
        rows = np.concatenate(rows) if rows else np.zeros((0, n_feats))
        ds[edge_begin:edge_end, :] = merge_feature_rows(ids, rows, edge_begin, edge_end)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(merge_edge_features)
