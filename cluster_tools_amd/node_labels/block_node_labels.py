#! /usr/bin/env python
"""BlockNodeLabels: the overlaps of every block's fragments with a second label volume on the GPU
(cluster_tools/node_labels/block_node_labels.py:21-222; task surface, config keys, job config keys
and log lines unchanged).  The job replaces `ndist.computeAndSerializeLabelOverlaps` (:153-156):
one library handle per job, blocks read ahead on a thread, the rows of `Handle.label_overlaps`
written as one variable-length chunk at the block's chunk id (serialization.py).  The two skip
rules of `_labels_for_block` hold: a block whose fragments sum to 0 and, with an ignore label, a
block whose labels are all that label write nothing."""
import os

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class BlockNodeLabelsBase(luigi.Task):
    task_name = 'block_node_labels'
    src_file = os.path.abspath(__file__)

    ws_path = luigi.Parameter()
    ws_key = luigi.Parameter()
    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    ignore_label = luigi.IntParameter(default=None)
    prefix = luigi.Parameter(default='')
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        config.update({'ws_path': self.ws_path, 'ws_key': self.ws_key,
                       'input_path': self.input_path, 'input_key': self.input_key,
                       'block_shape': block_shape,
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'ignore_label': self.ignore_label})
        shape = vu.get_shape(self.ws_path, self.ws_key)
        chunks = tuple(min(bs, sh) for bs, sh in zip(block_shape, shape))
        try:
            max_id = vu.file_reader(self.ws_path, 'r')[self.ws_key].attrs['maxId']
        except KeyError:
            raise KeyError("Dataset %s:%s does not have attribute maxId" % (self.ws_path, self.ws_key))
        # the overlap dataset: a chunk per block; MergeNodeLabels reads maxId from it
        with vu.file_reader(self.output_path) as f:
            ds_out = f.require_dataset(self.output_key, shape=shape, dtype='uint64', chunks=chunks,
                                       compression='gzip')
            ds_out.attrs['maxId'] = int(max_id)
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
        return luigi.LocalTarget(os.path.join(self.tmp_folder, self.task_name + '_%s.log' % self.prefix))


class BlockNodeLabelsLocal(BlockNodeLabelsBase, LocalTask):
    pass


class BlockNodeLabelsSlurm(BlockNodeLabelsBase, SlurmTask):
    pass


class BlockNodeLabelsLSF(BlockNodeLabelsBase, LSFTask):
    pass


#
# Implementation
#

def run_label_blocks(blocking, block_list, ds_ws, labels, ds_out, ignore_label):
    """The overlaps of every block of the job."""
    from cluster_tools_amd import ctws
    from cluster_tools_amd.node_labels.serialization import serialize_overlaps

    def read(block_id):
        bb = vu.block_to_bb(blocking.getBlock(block_id))
        ws = ds_ws[bb]
        if ws.sum() == 0:
            return ws, None
        return ws, labels[bb].astype('uint64')

    with ctws.Handle(fu.device()) as h, fu.read_ahead(read, block_list) as ahead:
        for block_id, nxt in ahead:
            fu.log("start processing block %i" % block_id)
            ws, labs = nxt.result()
            if labs is None:
                fu.log("block %i is empty" % block_id)
                fu.log_block_success(block_id)
                continue
            if ignore_label is not None and \
                    np.sum(labs == np.uint64(int(ignore_label) & 0xFFFFFFFFFFFFFFFF)) == labs.size:
                fu.log("labels of block %i is empty" % block_id)
                fu.log_block_success(block_id)
                continue
            chunk_id = fu.chunk_id(blocking.getBlock(block_id), blocking)
            rows = h.label_overlaps(np.ascontiguousarray(ws, dtype='uint64'), labs, ignore_label)
            ds_out.write_chunk(chunk_id, serialize_overlaps(rows), True)
            fu.log_block_success(block_id)


def block_node_labels(job_id, config_path):
    config = fu.load_config(job_id, config_path)
    block_shape = config['block_shape']
    block_list = config['block_list']
    ignore_label = config['ignore_label']
    with vu.file_reader(config['ws_path'], 'r') as f_in, vu.file_reader(config['input_path'], 'r') as f_lab, \
            vu.file_reader(config['output_path']) as f_out:
        ds_ws = f_in[config['ws_key']]
        ds_labels = f_lab[config['input_key']]
        shape, lab_shape = tuple(ds_ws.shape), tuple(ds_labels.shape)
        blocking = Blocking([0, 0, 0], list(shape), list(block_shape))
        # a label volume smaller than the fragments is read through nearest-neighbour interpolation
        if any(lsh < sh for lsh, sh in zip(lab_shape, shape)):
            assert not any(lsh > sh for lsh, sh in zip(lab_shape, shape)), \
                "Can't have label shape bigger then volshape"
            labels = vu.InterpolatedVolume(ds_labels, shape, spline_order=0)
        else:
            assert lab_shape == shape, "%s, %s" % (str(lab_shape), shape)
            labels = ds_labels
        if ignore_label is None:
            fu.log("accumulating labels without ignore label")
        else:
            fu.log("accumulating labels with ignore label %i" % ignore_label)
        run_label_blocks(blocking, block_list, ds_ws, labels, f_out[config['output_key']], ignore_label)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(block_node_labels)
