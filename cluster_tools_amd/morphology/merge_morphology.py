#! /usr/bin/env python
"""MergeMorphology: the blocks' tables into the table of the whole volume
(cluster_tools/morphology/merge_morphology.py:20-139; task surface, config keys, job config keys,
the label ranges of min(number_of_labels, 100000) dealt to max_jobs jobs and log lines unchanged).
The job replaces `ndist.mergeAndSerializeMorphology` (:129-131): it reads every written chunk of
the block dataset in ascending block-id order and, for the ids of each of its label ranges,

    size = sum of the blocks' sizes
    com  = (sum over the blocks, in that order, of float64(size_b) * com_b) / size
    min, max over the blocks' rows

An id without a row gets eleven zeros; a row whose id is number_of_labels or more is an error.
These are id tables, not voxels: vectorised numpy on the host.  Restated (nifty is not
available): DESIGN.md section 3.7."""
import os
from itertools import product

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class MergeMorphologyBase(luigi.Task):
    task_name = 'merge_morphology'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    number_of_labels = luigi.IntParameter()
    prefix = luigi.Parameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        out_shape = (int(self.number_of_labels), 11)
        out_chunks = (min(int(self.number_of_labels), 100000), 11)
        block_list = vu.blocks_in_volume([out_shape[0]], [out_chunks[0]])
        with vu.file_reader(self.output_path) as f:
            f.require_dataset(self.output_key, shape=out_shape, chunks=out_chunks, compression='gzip',
                              dtype='float64')
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'out_shape': out_shape, 'out_chunks': out_chunks})
        self.prepare_jobs(self.max_jobs, block_list, config, self.prefix)
        self.submit_jobs(self.max_jobs, self.prefix)
        self.wait_for_jobs(self.prefix)
        self.check_jobs(self.max_jobs, self.prefix)

    def output(self):
        return luigi.LocalTarget(os.path.join(self.tmp_folder, self.task_name + '_%s.log' % self.prefix))


class MergeMorphologyLocal(MergeMorphologyBase, LocalTask):
    pass


class MergeMorphologySlurm(MergeMorphologyBase, SlurmTask):
    pass


class MergeMorphologyLSF(MergeMorphologyBase, LSFTask):
    pass


#
# Implementation
#

def read_block_rows(ds_in, number_of_labels):
    """The rows of every written chunk of the block dataset, concatenated in ascending block-id
    order (the C order of the chunk ids)."""
    from cluster_tools_amd.morphology.serialization import read_morphology_rows, N_COLS
    out = []
    for cid in product(*[range(n) for n in ds_in.chunks_per_dimension]):
        rows = read_morphology_rows(ds_in, cid)
        if not len(rows):
            continue
        if rows[:, 0].max() >= number_of_labels:
            raise RuntimeError("merge_morphology: id %i in chunk %s of %s, but number_of_labels is %i"
                               % (int(rows[:, 0].max()), cid, ds_in.path, number_of_labels))
        out.append(rows)
    return np.concatenate(out) if out else np.zeros((0, N_COLS), dtype='float64')


def merge_rows(rows, label_begin, label_end):
    """The merged table (label_end - label_begin, 11) of the ids [label_begin, label_end) from the
    blocks' rows (in block order); ids without a row get zeros."""
    n_ids = label_end - label_begin
    out = np.zeros((n_ids, 11), dtype='float64')
    rows = rows[(rows[:, 0] >= label_begin) & (rows[:, 0] < label_end)]
    if not len(rows):
        return out
    idx = rows[:, 0].astype('int64') - label_begin
    # (bincount adds its weights in input order: the blocks' order)
    size = np.bincount(idx, weights=rows[:, 1], minlength=n_ids)
    have = size > 0
    out[have, 0] = np.arange(label_begin, label_end, dtype='float64')[have]
    out[:, 1] = size
    for a in (2, 3, 4):
        s = np.bincount(idx, weights=rows[:, 1] * rows[:, a], minlength=n_ids)
        out[have, a] = s[have] / size[have]
    lo = np.full((n_ids, 3), np.inf)
    hi = np.full((n_ids, 3), -np.inf)
    np.minimum.at(lo, idx, rows[:, 5:8])
    np.maximum.at(hi, idx, rows[:, 8:11])
    out[have, 5:8] = lo[have]
    out[have, 8:11] = hi[have]
    return out


def merge_morphology(job_id, config_path):
    config = fu.load_config(job_id, config_path)
    block_list = config['block_list']
    out_shape, out_chunks = config['out_shape'], config['out_chunks']
    blocking = Blocking([0], list(out_shape[:1]), list(out_chunks[:1]))
    with vu.file_reader(config['input_path'], 'r') as f_in, vu.file_reader(config['output_path']) as f_out:
        ds_out = f_out[config['output_key']]
        rows = read_block_rows(f_in[config['input_key']], int(out_shape[0])) if block_list else None
        for block_id in block_list:
            block = blocking.getBlock(block_id)
            label_begin, label_end = int(block.begin[0]), int(block.end[0])
            ds_out[label_begin:label_end, :] = merge_rows(rows, label_begin, label_end)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(merge_morphology)
