#! /usr/bin/env python
"""FillingSizeFilter: the ids in discard_ids.npy are regrown from their neighbours by a seeded
watershed on a height map, block by block on the GPU (cluster_tools/postprocess/
filling_size_filter.py:17-199; task surface, config keys and log lines unchanged).

The reference's job cannot run as written; this builds its evident intent:
`hmap_bb` is undefined for a 3-D height map (`bb` is used), a 4-D height map gives its channel 0,
the uint64 labels are flooded as order-preserving compact ids and mapped back (vigra on
labels.astype('uint32') wherever that cast is lossless), and 'maxId' is copied as
BackgroundSizeFilter copies it."""
import os

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask
from cluster_tools_amd.postprocess.background_size_filter import parse_discard_path, run_filter_job


class FillingSizeFilterBase(luigi.Task):
    task_name = 'filling_size_filter'
    src_file = os.path.abspath(__file__)

    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    hmap_path = luigi.Parameter()
    hmap_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def _parse_log(self, log_path):
        return parse_discard_path(log_path)

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        shape = vu.get_shape(self.input_path, self.input_key)
        block_list = self.blocks_to_process(shape, block_shape, roi_begin, roi_end)
        # chunks as BackgroundSizeFilter chooses them (half a block; an existing dataset keeps its
        # own): the reference's fixed (25, 256, 256) does not divide the blocks, so jobs would
        # rewrite each other's chunks and the Write task of the relabel refuses such a dataset
        chunks = tuple(min(bs // 2, sh) for bs, sh in zip(block_shape, shape))
        with vu.file_reader(self.output_path) as f:
            if self.output_key in f:
                chunks = f[self.output_key].chunks
            f.require_dataset(self.output_key, shape=shape, chunks=chunks, dtype='uint64', compression='gzip')
        # the job config holds the paths only, as in the reference
        config = {'input_path': self.input_path, 'input_key': self.input_key,
                  'output_path': self.output_path, 'output_key': self.output_key,
                  'hmap_path': self.hmap_path, 'hmap_key': self.hmap_key,
                  'block_shape': block_shape, 'res_path': self._parse_log(self.input().path)}
        self.run_jobs(min(len(block_list), self.max_jobs), block_list, config)


class FillingSizeFilterLocal(FillingSizeFilterBase, LocalTask):
    pass


class FillingSizeFilterSlurm(FillingSizeFilterBase, SlurmTask):
    pass


class FillingSizeFilterLSF(FillingSizeFilterBase, LSFTask):
    pass


def filling_size_filter(job_id, config_path):
    config = fu.load_config(job_id, config_path)
    run_filter_job(job_id, config, with_hmap=True)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(filling_size_filter)
