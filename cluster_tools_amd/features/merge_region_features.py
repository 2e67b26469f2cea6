#! /usr/bin/env python
"""MergeRegionFeatures: the blocks' [id, count, mean] rows into the mean table of the whole volume
(cluster_tools/features/merge_region_features.py:16-170; task surface, config keys, job config keys,
the label ranges of min(10000, number_of_labels) dealt consecutively to max_jobs jobs, the output
dataset -- float32, (number_of_labels,), chunks (min(10000, number_of_labels),), gzip -- and the log
lines unchanged).  The job reads every written chunk of the temporary block dataset once, in
ascending block-id order, and for the ids of its label range

    count = sum of the blocks' counts
    mean  = (sum over the blocks, in that order, of float64(count_b) * mean_b) / count

cast once to float32.  An id whose total count is 0 -- the ignore label, an id that occurs nowhere
-- gets 0; a row whose id is number_of_labels or more is an error.  The reference keeps a float32
running average instead (:122-127); the two agree within float32 rounding.
These are id tables, not voxels: vectorised numpy on the host."""
import os
from itertools import product

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class MergeRegionFeaturesBase(luigi.Task):
    task_name = 'merge_region_features'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    number_of_labels = luigi.IntParameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        number_of_labels = int(self.number_of_labels)
        chunk_size = min(10000, number_of_labels)
        with vu.file_reader(self.output_path) as f:
            f.require_dataset(self.output_key, dtype='float32', shape=(number_of_labels,),
                              chunks=(chunk_size,), compression='gzip')
        tmp_path = os.path.join(self.tmp_folder, 'region_features_tmp.n5')
        tmp_key = 'block_feats'
        config.update({'output_path': self.output_path, 'output_key': self.output_key,
                       'tmp_path': tmp_path, 'tmp_key': tmp_key,
                       'node_chunk_size': chunk_size})
        node_block_list = vu.blocks_in_volume([number_of_labels], [chunk_size])
        n_jobs = min(len(node_block_list), self.max_jobs)
        self.prepare_jobs(n_jobs, node_block_list, config, consecutive_blocks=True)
        self.submit_jobs(n_jobs)
        self.wait_for_jobs()
        self.check_jobs(n_jobs)


class MergeRegionFeaturesLocal(MergeRegionFeaturesBase, LocalTask):
    pass


class MergeRegionFeaturesSlurm(MergeRegionFeaturesBase, SlurmTask):
    pass


class MergeRegionFeaturesLSF(MergeRegionFeaturesBase, LSFTask):
    pass


#
# Implementation
#

def read_block_rows(ds_in, number_of_labels):
    """The rows of every written chunk of the block dataset, concatenated in ascending block-id
    order (the C order of the chunk ids)."""
    from cluster_tools_amd.features.region_serialization import read_region_feature_rows, N_COLS
    out = []
    for cid in product(*[range(n) for n in ds_in.chunks_per_dimension]):
        rows = read_region_feature_rows(ds_in, cid)
        if not len(rows):
            continue
        if rows[:, 0].max() >= number_of_labels:
            raise RuntimeError("merge_region_features: id %i in chunk %s of %s, but number_of_labels is %i"
                               % (int(rows[:, 0].max()), cid, ds_in.path, number_of_labels))
        out.append(rows)
    return np.concatenate(out) if out else np.zeros((0, N_COLS), dtype='float64')


def merge_rows(rows, node_begin, node_end):
    """The merged means (node_end - node_begin,) float32 of the ids [node_begin, node_end) from the
    blocks' rows (in block order); ids whose total count is 0 get 0."""
    n_ids = node_end - node_begin
    out = np.zeros(n_ids, dtype='float64')
    rows = rows[(rows[:, 0] >= node_begin) & (rows[:, 0] < node_end)]
    if len(rows):
        idx = rows[:, 0].astype('int64') - node_begin
        # (bincount adds its weights in input order: the blocks' order)
        count = np.bincount(idx, weights=rows[:, 1], minlength=n_ids)
        total = np.bincount(idx, weights=rows[:, 1] * rows[:, 2], minlength=n_ids)
        have = count > 0
        out[have] = total[have] / count[have]
    return out.astype('float32')


def merge_region_features(job_id, config_path):
    config = fu.load_config(job_id, config_path)
    node_block_list = config['block_list']
    node_chunk_size = config['node_chunk_size']
    with vu.file_reader(config['output_path']) as f, vu.file_reader(config['tmp_path'], 'r') as f_in:
        ds = f[config['output_key']]
        n_nodes = int(ds.shape[0])
        if node_block_list:
            node_blocking = Blocking([0], [n_nodes], [node_chunk_size])
            node_begin = int(node_blocking.getBlock(node_block_list[0]).begin[0])
            node_end = int(node_blocking.getBlock(node_block_list[-1]).end[0])
            fu.log("processing node range %i to %i" % (node_begin, node_end))
            rows = read_block_rows(f_in[config['tmp_key']], n_nodes)
            ds[node_begin:node_end] = merge_rows(rows, node_begin, node_end)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(merge_region_features)
