#! /usr/bin/env python
"""BlockMorphology: size, centre of mass and bounding box of every id of every block on the GPU
(cluster_tools/morphology/block_morphology.py:20-175; task surface, config keys, job config keys
and log lines unchanged).  The job replaces `ndist.computeAndSerializeMorphology` (:133-135): one
library handle per job, blocks read ahead on a thread, the rows of `Handle.block_morphology`
written as one variable-length float64 chunk at the block's chunk id (serialization.py).  The skip
rule of `_morphology_for_block` holds: a block whose labels sum to 0 writes nothing."""
import os

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class BlockMorphologyBase(luigi.Task):
    task_name = 'block_morphology'
    src_file = os.path.abspath(__file__)

    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    prefix = luigi.Parameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'block_shape': block_shape,
                       'output_path': self.output_path, 'output_key': self.output_key})
        shape = vu.get_shape(self.input_path, self.input_key)
        # the block dataset: a variable-length chunk per block
        with vu.file_reader(self.output_path) as f:
            f.require_dataset(self.output_key, shape=shape, dtype='float64', chunks=tuple(block_shape),
                              compression='gzip')
        if self.n_retries == 0:
            block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        else:
            block_list = self.block_list
            self.clean_up_for_retry(block_list)
        n_jobs = min(len(block_list), self.max_jobs)
        self.prepare_jobs(n_jobs, block_list, config, self.prefix)
        self.submit_jobs(n_jobs, self.prefix)
        self.wait_for_jobs()
        self.check_jobs(n_jobs, self.prefix)

    def output(self):
        return luigi.LocalTarget(os.path.join(self.tmp_folder, "%s_%s.log" % (self.task_name, self.prefix)))


class BlockMorphologyLocal(BlockMorphologyBase, LocalTask):
    pass


class BlockMorphologySlurm(BlockMorphologyBase, SlurmTask):
    pass


class BlockMorphologyLSF(BlockMorphologyBase, LSFTask):
    pass


#
# Implementation
#

def run_morphology_blocks(blocking, block_list, ds_in, ds_out):
    """The morphology table of every block of the job."""
    from cluster_tools_amd import ctws
    from cluster_tools_amd.morphology.serialization import serialize_morphology

    def read(block_id):
        return ds_in[vu.block_to_bb(blocking.getBlock(block_id))]

    with ctws.Handle(fu.device()) as h, fu.read_ahead(read, block_list) as ahead:
        for block_id, nxt in ahead:
            fu.log("start processing block %i" % block_id)
            seg = nxt.result()
            if seg.sum() == 0:
                fu.log("block %i is empty" % block_id)
                fu.log_block_success(block_id)
                continue
            block = blocking.getBlock(block_id)
            rows = h.block_morphology(np.ascontiguousarray(seg, dtype='uint64'), [int(b) for b in block.begin])
            ds_out.write_chunk(fu.chunk_id(block, blocking), serialize_morphology(rows), True)
            fu.log_block_success(block_id)


def block_morphology(job_id, config_path):
    config = fu.load_config(job_id, config_path)
    block_shape = config['block_shape']
    block_list = config['block_list']
    with vu.file_reader(config['input_path'], 'r') as f_in, vu.file_reader(config['output_path']) as f_out:
        ds_in = f_in[config['input_key']]
        blocking = Blocking([0, 0, 0], list(ds_in.shape), list(block_shape))
        run_morphology_blocks(blocking, block_list, ds_in, f_out[config['output_key']])
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(block_morphology)
