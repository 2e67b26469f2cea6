#! /usr/bin/env python
"""SizeFilterBlocks: the ids whose voxel count over the whole volume is below size_threshold
(cluster_tools/postprocess/size_filter_blocks.py:19-113; task surface, config keys, log lines and
temp files unchanged).  One job merges the (unique, count) tables FindUniques(return_counts=True)
wrote per job -- id tables, not voxels -- on the host with a sort and reduceat; the reference's
dense `zeros(max_id + 1)` count array cannot hold un-relabelled watershed ids
(block_id * prod(block_shape) + k)."""
import os

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class SizeFilterBlocksBase(luigi.Task):
    task_name = 'size_filter_blocks'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    size_threshold = luigi.IntParameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        shape = vu.get_shape(self.input_path, self.input_key)
        block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        # one job merges the find_uniques results of the n_jobs jobs of the previous task
        config = {'tmp_folder': self.tmp_folder, 'n_jobs': min(len(block_list), self.max_jobs),
                  'size_threshold': self.size_threshold}
        self.prepare_jobs(1, None, config)
        self.submit_jobs(1)
        self.wait_for_jobs()
        # the filter tasks read the path from the third-last line of this log (`_parse_log`)
        self._write_log("saving results to %s" % os.path.join(self.tmp_folder, 'discard_ids.npy'))
        self.check_jobs(1)


class SizeFilterBlocksLocal(SizeFilterBlocksBase, LocalTask):
    pass


class SizeFilterBlocksSlurm(SizeFilterBlocksBase, SlurmTask):
    pass


class SizeFilterBlocksLSF(SizeFilterBlocksBase, LSFTask):
    pass


def merge_counts(unique_values, count_values):
    """The jobs' (unique, count) tables -> (global sorted uniques, summed counts), uint64."""
    allv = np.concatenate([np.asarray(u, dtype='uint64') for u in unique_values])
    allc = np.concatenate([np.asarray(c, dtype='uint64') for c in count_values])
    assert allv.shape == allc.shape, "%s, %s" % (allv.shape, allc.shape)
    if len(allv) == 0:
        return allv, allc
    order = np.argsort(allv, kind='stable')
    allv, allc = allv[order], allc[order]
    uniques, starts = np.unique(allv, return_index=True)
    return uniques, np.add.reduceat(allc, starts).astype('uint64')


def size_filter_blocks(job_id, config_path):
    config = fu.load_config(job_id, config_path)
    tmp_folder = config['tmp_folder']
    size_threshold = config['size_threshold']
    unique_values = [np.load(os.path.join(tmp_folder, 'find_uniques_job_%i.npy' % j)) for j in range(config['n_jobs'])]
    count_values = [np.load(os.path.join(tmp_folder, 'counts_job_%i.npy' % j)) for j in range(config['n_jobs'])]
    uniques, counts = merge_counts(unique_values, count_values)
    fu.log("applying size filter %i" % size_threshold)
    # (0 is discarded too when the background is that small, as in the reference)
    discard_ids = uniques[counts < size_threshold]
    fu.log("discarding %i / %i ids" % (len(discard_ids), len(uniques)))
    save_path = os.path.join(tmp_folder, 'discard_ids.npy')
    fu.log("saving results to %s" % save_path)
    np.save(save_path, discard_ids)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(size_filter_blocks)
