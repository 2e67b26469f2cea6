#! /usr/bin/env python
"""RegionFeatures: the number of voxels and the mean input value of every id of every block on the
GPU (cluster_tools/features/region_features.py:26-212; task surface, config keys, job config keys,
the temporary dataset's path, key, shape and chunks and the log lines unchanged; the temporary
dataset is float64, region_serialization.py).  The job replaces
`vigra.analysis.extractRegionFeatures(vu.normalize(input), labels, ['mean', 'count'], ignoreLabel)`
(:143-149): one library handle per job, blocks read ahead on a thread, the rows of
`Handle.region_features_block` written as one variable-length chunk at the block's chunk id.  The
skip rule of `_block_features` holds: with an ignore label, a block that holds nothing else writes
nothing.  A 4-D (multi-channel) input is the reference's own TODO and is refused before any job
starts."""
import os

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class RegionFeaturesBase(luigi.Task):
    task_name = 'region_features'
    src_file = os.path.abspath(__file__)

    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    labels_path = luigi.Parameter()
    labels_key = luigi.Parameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'ignore_label': 0})
        return config

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        output_path = os.path.join(self.tmp_folder, 'region_features_tmp.n5')
        output_key = 'block_feats'
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'labels_path': self.labels_path, 'labels_key': self.labels_key,
                       'output_path': output_path, 'output_key': output_key,
                       'block_shape': block_shape})
        shape = vu.get_shape(self.input_path, self.input_key)
        if len(shape) != 3:
            raise NotImplementedError("region_features: the input %s:%s has %i dimensions; multi-channel inputs "
                                      "are not supported" % (self.input_path, self.input_key, len(shape)))
        # the temporary block dataset: a variable-length chunk per block
        with vu.file_reader(output_path) as f:
            f.require_dataset(output_key, shape=shape, compression='gzip', chunks=tuple(block_shape),
                              dtype='float64')
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


class RegionFeaturesLocal(RegionFeaturesBase, LocalTask):
    pass


class RegionFeaturesSlurm(RegionFeaturesBase, SlurmTask):
    pass


class RegionFeaturesLSF(RegionFeaturesBase, LSFTask):
    pass


#
# Implementation
#

def run_region_feature_blocks(blocking, block_list, ds_in, ds_labels, ds_out, ignore_label):
    """The [id, count, mean] table of every block of the job."""
    from cluster_tools_amd import ctws
    from cluster_tools_amd.features.region_serialization import serialize_region_features

    def read(block_id):
        bb = vu.block_to_bb(blocking.getBlock(block_id))
        return ds_labels[bb], ds_in[bb]

    with ctws.Handle(fu.device()) as h, fu.read_ahead(read, block_list) as ahead:
        for block_id, nxt in ahead:
            fu.log("start processing block %i" % block_id)
            labels, data = nxt.result()
            if ignore_label is not None and not (labels != ignore_label).any():
                fu.log_block_success(block_id)
                continue
            chunk_id = fu.chunk_id(blocking.getBlock(block_id), blocking)
            rows = h.region_features_block(np.ascontiguousarray(labels, dtype='uint64'), data, ignore_label)
            ds_out.write_chunk(chunk_id, serialize_region_features(rows), True)
            fu.log_block_success(block_id)


def region_features(job_id, config_path):
    config = fu.load_config(job_id, config_path)
    block_list = config['block_list']
    block_shape = config['block_shape']
    ignore_label = config['ignore_label']
    with vu.file_reader(config['input_path'], 'r') as f_in, vu.file_reader(config['labels_path'], 'r') as f_l, \
            vu.file_reader(config['output_path']) as f_out:
        ds_out = f_out[config['output_key']]
        blocking = Blocking([0, 0, 0], list(ds_out.shape), list(block_shape))
        run_region_feature_blocks(blocking, block_list, f_in[config['input_key']], f_l[config['labels_key']],
                                  ds_out, ignore_label)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(region_features)
