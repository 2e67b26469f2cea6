#! /usr/bin/env python
"""MapEdgeIds: for every block of a scale, the index of each of its edges in the global edge
list, as the dataset `edgeIds` of the block's group (cluster_tools/graph/map_edge_ids.py:20-120,
`ndist.mapEdgeIds` :94-113; parameters, config keys and log lines unchanged).  These are id
tables, not voxels: one job on the host (ranks of the node ids + searchsorted), as
SizeFilterBlocks merges its tables.  The dataset name is nifty's, recalled, not pinned."""
import os

import numpy as np

from cluster_tools_amd import luigi_compat as luigi
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.cluster_tasks import SlurmTask, LocalTask, LSFTask


class MapEdgeIdsBase(luigi.Task):
    task_name = 'map_edge_ids'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    graph_path = luigi.Parameter()
    input_key = luigi.Parameter()
    scale = luigi.IntParameter()
    dependency = luigi.TaskParameter()

    def requires(self):
        return self.dependency

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        with vu.file_reader(self.graph_path) as f:
            shape = f.attrs['shape']
        factor = 2 ** self.scale
        block_shape = tuple(sh * factor for sh in block_shape)
        block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        config.update({'graph_path': self.graph_path, 'scale': self.scale, 'input_key': self.input_key})
        self.prepare_jobs(1, block_list, config)
        self.submit_jobs(1)
        self.wait_for_jobs()
        self.check_jobs(1)

    def output(self):
        return luigi.LocalTarget(os.path.join(self.tmp_folder, self.task_name + '_s%i.log' % self.scale))


class MapEdgeIdsLocal(MapEdgeIdsBase, LocalTask):
    pass


class MapEdgeIdsSlurm(MapEdgeIdsBase, SlurmTask):
    pass


class MapEdgeIdsLSF(MapEdgeIdsBase, LSFTask):
    pass


#
# Implementation
#

class EdgeIndex:
    """The global edge list (M, 2), lexicographically sorted, as one ascending uint64 key per
    edge: rank(u) * n + rank(v) over its n distinct node ids (n < 2^32)."""

    def __init__(self, global_edges):
        edges = np.asarray(global_edges, dtype='uint64').reshape(-1, 2)
        self.nodes = np.unique(edges)
        assert len(self.nodes) < 2 ** 32, len(self.nodes)
        self.keys = self._keys(edges)
        assert np.all(self.keys[1:] > self.keys[:-1]), "the global edges are not sorted and unique"

    def _keys(self, edges):
        ranks = np.searchsorted(self.nodes, edges).astype('uint64')
        return ranks[:, 0] * np.uint64(max(len(self.nodes), 1)) + ranks[:, 1]

    def edge_ids(self, block_edges):
        """edgeIds[i] = the index of block edge i in the global list."""
        edges = np.asarray(block_edges, dtype='uint64').reshape(-1, 2)
        if len(edges) == 0:
            return np.zeros(0, dtype='uint64')
        known = np.isin(edges, self.nodes).all(axis=1)
        ids = np.searchsorted(self.keys, self._keys(edges))
        known &= ids < len(self.keys)
        known[known] = self.keys[ids[known]] == self._keys(edges[known])
        if not known.all():
            raise RuntimeError("%i block edges are not in the global graph, first %s"
                               % (int((~known).sum()), edges[~known][0].tolist()))
        return ids.astype('uint64')


def map_edge_ids(job_id, config_path):
    from cluster_tools_amd.graph.serialization import read_table, write_edge_ids
    config = fu.load_config(job_id, config_path)
    block_prefix = 's%i/sub_graphs/block_' % config['scale']
    with vu.file_reader(config['graph_path']) as f:
        index = EdgeIndex(read_table(f[config['input_key']], 'edges', 2))
        for block_id in config['block_list']:
            key = block_prefix + str(block_id)
            write_edge_ids(f, key, index.edge_ids(read_table(f[key], 'edges', 2)))
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(map_edge_ids)
