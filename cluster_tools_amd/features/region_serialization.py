"""The on-disk form of block region features: one variable-length n5 chunk
of float64 per block at `chunk_id = block.begin // block_shape` of
`region_features_tmp.n5/block_feats`.  A chunk is the flat sequence of its m x 3 table

    id, count, mean

sorted by id, so `data[::3]`, `data[1::3]` and `data[2::3]` read the columns as they do in the
reference (region_features.py:155-166).  The reference writes float32 there, which cannot hold an
id from 2^24 on; the dataset is private to RegionFeatures and MergeRegionFeatures."""
import numpy as np

N_COLS = 3


def serialize_region_features(rows):
    """rows (m, 3) float64 -> the flat sequence."""
    rows = np.ascontiguousarray(rows, dtype='float64')
    if rows.ndim != 2 or rows.shape[1] != N_COLS:
        raise ValueError("region feature rows are (m, %i), not %s" % (N_COLS, rows.shape))
    return rows.reshape(-1)


def deserialize_region_features(flat):
    """The flat sequence -> rows (m, 3) float64."""
    flat = np.asarray(flat, dtype='float64').ravel()
    if len(flat) % N_COLS:
        raise ValueError("region feature chunk: %i values are no whole number of rows of %i" % (len(flat), N_COLS))
    return flat.reshape(-1, N_COLS)


def read_region_feature_rows(ds, chunk_id):
    """The rows of one chunk of an open block-feature dataset; a chunk that was not written has none."""
    flat = ds.read_chunk(tuple(int(c) for c in chunk_id))
    if flat is None:
        return np.zeros((0, N_COLS), dtype='float64')
    if flat.ndim != 1:
        raise ValueError("chunk %s of %s is no variable-length region feature chunk" % (tuple(chunk_id), ds.path))
    return deserialize_region_features(flat)
