"""The on-disk form of block morphology: one variable-length n5 chunk of
float64 per block, as the reference's `ndist.computeAndSerializeMorphology` writes it at
`chunk_id = block.begin // block_shape`.  A chunk is the flat sequence of its m x 11 table

    id, size, com_z, com_y, com_x, min_z, min_y, min_x, max_z, max_y, max_x

sorted by id, in global coordinates, minima and maxima inclusive.

nifty is not available, so byte parity with nifty's chunks is not pinned; the readers and writers
of this package agree with each other."""
import numpy as np

N_COLS = 11


def serialize_morphology(rows):
    """rows (m, 11) float64 -> the flat sequence."""
    rows = np.ascontiguousarray(rows, dtype='float64')
    if rows.ndim != 2 or rows.shape[1] != N_COLS:
        raise ValueError("morphology rows are (m, %i), not %s" % (N_COLS, rows.shape))
    return rows.reshape(-1)


def deserialize_morphology(flat):
    """The flat sequence -> rows (m, 11) float64."""
    flat = np.asarray(flat, dtype='float64').ravel()
    if len(flat) % N_COLS:
        raise ValueError("morphology chunk: %i values are no whole number of rows of %i" % (len(flat), N_COLS))
    return flat.reshape(-1, N_COLS)


def read_morphology_rows(ds, chunk_id):
    """The rows of one chunk of an open block-morphology dataset; a chunk that was not written has none."""
    flat = ds.read_chunk(tuple(int(c) for c in chunk_id))
    if flat is None:
        return np.zeros((0, N_COLS), dtype='float64')
    if flat.ndim != 1:
        raise ValueError("chunk %s of %s is no variable-length morphology chunk" % (tuple(chunk_id), ds.path))
    return deserialize_morphology(flat)
