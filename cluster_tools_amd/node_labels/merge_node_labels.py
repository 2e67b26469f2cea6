#! /usr/bin/env python
"""MergeNodeLabels: the blocks' overlaps into the overlaps of every node
(cluster_tools/node_labels/merge_node_labels.py:20-159; task surface, config keys, job config keys,
the node ranges of min(n_labels, 100000) and log lines unchanged).  The job replaces
`ndist.mergeAndSerializeOverlaps` (:145-151): the rows of a node range are gathered from every
block chunk, the counts of equal (node, label) rows are summed on the GPU
(`Handle.unique_pairs_u64` with weights) and the result is written

  max_overlap=True    into the 1-D uint64 dataset: out[node] = the label of the largest count, the
                      smallest label among tied ones; a node without a counted voxel gets the
                      ignore label (0 when that is None)
  max_overlap=False   as one variable-length chunk per node range (serialization.py), with counts
                      iff serialize_counts

max_overlap=True with serialize_counts=True has no form in the 1-D dataset and is refused before
any job starts.  Restated (nifty is not available): DESIGN.md section 3.6."""
import os
from itertools import product

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


def check_supported(max_overlap, serialize_counts):
    if max_overlap and serialize_counts:
        raise NotImplementedError("merge_node_labels: max_overlap and serialize_counts are both set, but the "
                                  "max-overlap output is a 1-D dataset of one label per node and has no place "
                                  "for counts; set max_overlap=False to serialize the counts")


class MergeNodeLabelsBase(luigi.Task):
    task_name = 'merge_node_labels'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    output_path = luigi.Parameter()
    output_key = luigi.Parameter()
    max_overlap = luigi.BoolParameter(default=True)
    ignore_label = luigi.IntParameter(default=None)
    serialize_counts = luigi.BoolParameter(default=False)
    prefix = luigi.Parameter(default='')
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def _job_prefix(self):
        return ('max_ol' if self.max_overlap else 'all_ol') + '_%s' % self.prefix

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        check_supported(self.max_overlap, self.serialize_counts)
        config = self.get_task_config()
        with vu.file_reader(self.input_path, 'r') as f:
            number_of_labels = int(f[self.input_key].attrs['maxId']) + 1
        node_shape = (number_of_labels,)
        node_chunks = (min(number_of_labels, 100000),)
        block_list = vu.blocks_in_volume(node_shape, node_chunks)
        with vu.file_reader(self.output_path) as f:
            ds = f.require_dataset(self.output_key, shape=node_shape, chunks=node_chunks, compression='gzip',
                                   dtype='uint64')
            if not self.max_overlap:
                from cluster_tools_amd.node_labels.serialization import COUNTS_ATTR
                ds.attrs[COUNTS_ATTR] = bool(self.serialize_counts)
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'max_overlap': self.max_overlap, 'node_shape': node_shape, 'node_chunks': node_chunks,
                       'ignore_label': self.ignore_label, 'serialize_counts': self.serialize_counts})
        prefix = self._job_prefix()
        n_jobs = min(self.max_jobs, len(block_list))
        self.prepare_jobs(n_jobs, block_list, config, prefix)
        self.submit_jobs(n_jobs, prefix)
        self.wait_for_jobs(prefix)
        self.check_jobs(n_jobs, prefix)

    def output(self):
        return luigi.LocalTarget(os.path.join(self.tmp_folder, self.task_name + '_%s.log' % self._job_prefix()))


class MergeNodeLabelsLocal(MergeNodeLabelsBase, LocalTask):
    pass


class MergeNodeLabelsSlurm(MergeNodeLabelsBase, SlurmTask):
    pass


class MergeNodeLabelsLSF(MergeNodeLabelsBase, LSFTask):
    pass


#
# Implementation
#

def max_overlap_labels(rows, label_begin, label_end, ignore_label):
    """out[node - label_begin] = the label of the largest count among the merged rows (m, 3) of the
    nodes [label_begin, label_end), the smallest label among tied ones; a node without a row gets
    the ignore label (0 when that is None).  An id table, not voxels: numpy on the host."""
    fill = 0 if ignore_label is None else int(ignore_label) & 0xFFFFFFFFFFFFFFFF
    out = np.full(label_end - label_begin, fill, dtype='uint64')
    if len(rows):
        # by node ascending, count descending, label ascending: a node's first row wins
        order = np.lexsort((rows[:, 1], np.iinfo('uint64').max - rows[:, 2], rows[:, 0]))
        rows = rows[order]
        first = np.ones(len(rows), dtype=bool)
        first[1:] = rows[1:, 0] != rows[:-1, 0]
        out[(rows[first, 0] - np.uint64(label_begin)).astype('int64')] = rows[first, 1]
    return out


def read_block_rows(ds_in):
    """The rows (node, label, count) of every block chunk of the overlap dataset, concatenated."""
    from cluster_tools_amd.node_labels.serialization import read_overlap_rows
    rows = [read_overlap_rows(ds_in, cid) for cid in product(*[range(n) for n in ds_in.chunks_per_dimension])]
    rows = [r for r in rows if len(r)]
    return np.concatenate(rows) if rows else np.zeros((0, 3), dtype='uint64')


def merge_node_labels(job_id, config_path):
    from cluster_tools_amd import ctws
    from cluster_tools_amd.node_labels.serialization import serialize_overlaps
    config = fu.load_config(job_id, config_path)
    max_overlap, serialize_counts = config['max_overlap'], config['serialize_counts']
    check_supported(max_overlap, serialize_counts)
    ignore_label = config['ignore_label']
    blocking = Blocking([0], list(config['node_shape']), list(config['node_chunks']))
    with vu.file_reader(config['input_path'], 'r') as f_in, vu.file_reader(config['output_path']) as f_out:
        rows = read_block_rows(f_in[config['input_key']])
        ds_out = f_out[config['output_key']]
        handle = None
        try:
            for block_id in config['block_list']:
                block = blocking.getBlock(block_id)
                label_begin, label_end = int(block.begin[0]), int(block.end[0])
                sel = rows[(rows[:, 0] >= np.uint64(label_begin)) & (rows[:, 0] < np.uint64(label_end))]
                if len(sel):
                    if handle is None:
                        handle = ctws.Handle(fu.device())
                    pairs, sums = handle.unique_pairs_u64(sel[:, :2], sel[:, 2])
                    sel = np.concatenate([pairs, sums[:, None]], axis=1)
                if max_overlap:
                    ds_out[label_begin:label_end] = max_overlap_labels(sel, label_begin, label_end, ignore_label)
                else:
                    ds_out.write_chunk((block_id,), serialize_overlaps(sel, serialize_counts), True)
        finally:
            if handle is not None:
                handle.close()
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(merge_node_labels)
