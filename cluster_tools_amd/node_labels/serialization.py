"""The on-disk form of label overlaps: one variable-length n5 chunk of
uint64 per block (BlockNodeLabels) or per node range (MergeNodeLabels, max_overlap=False), as the
reference's `ndist.computeAndSerializeLabelOverlaps` / `ndist.mergeAndSerializeOverlaps` write
them with `ds.write_chunk(..., True)`.

A chunk is a flat uint64 sequence.  For each node in ascending order:

    node, k, then k x (label, count)      with counts, labels ascending
    node, k, then k labels                 without counts (serialize_counts=False)

nifty is not available, so byte parity with nifty's chunks is not pinned; the readers and writers
of this package agree with each other and with `deserialize_overlap_chunk`, the shape in which the
reference's consumers call `ndist.deserializeOverlapChunk(path, chunk_id)[0]`."""
import numpy as np

from cluster_tools_amd.io.chunked import Dataset

COUNTS_ATTR = 'serializeCounts'  # on a merged dataset: whether its chunks carry counts


def serialize_overlaps(rows, with_counts=True):
    """rows (m, 3) uint64 of (node, label, count), sorted by (node, label) -> the flat sequence."""
    rows = np.ascontiguousarray(rows, dtype='uint64').reshape(-1, 3)
    if len(rows) == 0:
        return np.zeros(0, dtype='uint64')
    nodes, start, k = np.unique(rows[:, 0], return_index=True, return_counts=True)
    w = 2 if with_counts else 1
    sizes = 2 + w * k
    offs = np.cumsum(sizes) - sizes
    out = np.empty(int(sizes.sum()), dtype='uint64')
    out[offs] = nodes
    out[offs + 1] = k.astype('uint64')
    group = np.repeat(np.arange(len(nodes)), k)
    pos = offs[group] + 2 + w * (np.arange(len(rows)) - start[group])
    out[pos] = rows[:, 1]
    if with_counts:
        out[pos + 1] = rows[:, 2]
    return out


def deserialize_overlaps(flat, with_counts=True):
    """The flat sequence -> rows (m, 3) uint64; without counts the third column is 0."""
    flat = np.asarray(flat, dtype='uint64').ravel()
    w = 2 if with_counts else 1
    n = len(flat)
    heads, pos = [], 0
    while pos < n:
        if pos + 2 > n:
            raise ValueError("overlap chunk: truncated node header at element %i of %i" % (pos, n))
        heads.append(pos)
        pos += 2 + w * int(flat[pos + 1])
    if pos != n:
        raise ValueError("overlap chunk: the last node's entries end at element %i of %i" % (pos, n))
    if not heads:
        return np.zeros((0, 3), dtype='uint64')
    heads = np.array(heads, dtype='int64')
    k = flat[heads + 1].astype('int64')
    group = np.repeat(np.arange(len(heads)), k)
    start = np.cumsum(k) - k
    at = heads[group] + 2 + w * (np.arange(int(k.sum())) - start[group])
    rows = np.zeros((len(at), 3), dtype='uint64')
    rows[:, 0] = flat[heads][group]
    rows[:, 1] = flat[at]
    if with_counts:
        rows[:, 2] = flat[at + 1]
    return rows


def read_overlap_rows(ds, chunk_id, with_counts=True):
    """The rows of one chunk of an open overlap dataset; a chunk that was not written has none."""
    flat = ds.read_chunk(tuple(int(c) for c in chunk_id))
    if flat is None:
        return np.zeros((0, 3), dtype='uint64')
    if flat.ndim != 1:
        raise ValueError("chunk %s of %s is no variable-length overlap chunk" % (tuple(chunk_id), ds.path))
    return deserialize_overlaps(flat, with_counts)


def deserialize_overlap_chunk(ds_path, chunk_id):
    """(dict node -> dict label -> count, max_label) of one chunk of the overlap dataset at
    ds_path (the dataset's folder, as nifty takes it).  A chunk that was not written gives
    ({}, 0).  A merged dataset written without counts gives dict node -> dict label -> 0."""
    ds = Dataset(ds_path, 'n5')
    rows = read_overlap_rows(ds, chunk_id, bool(ds.attrs.get(COUNTS_ATTR, True)))
    out = {}
    for node, label, count in rows.tolist():
        out.setdefault(node, {})[label] = count
    return out, int(rows[:, 1].max()) if len(rows) else 0
