"""CPU restatement of the size filter's `apply_block` (postprocess/background_size_filter.py:110-130,
filling_size_filter.py:112-136) for the tests, on top of the oracle's watershed: np.isin marks
the discarded voxels, they are set to 0, np.unique(return_inverse) gives the order-preserving
compact ids, oracle.watershed floods the float32 height map from them (inside
oracle.flood_model(): the GPU's tie-break model; outside: vigra's heap order) and the result
is mapped back through the unique values.  Without any nonzero seed left the flood's own
labels (vigra's seeds from the strict minima, 1..n) are the output."""
import numpy as np

from oracle import oracle as O

ZERO, COPIED, WRITTEN, FAILED = 5, 6, 0, 4


def fragments(shape, seed=11):
    """DT-watershed fragments of the synthetic boundary map (ids 1..n) and the map."""
    from cluster_tools_amd.synthetic import boundary_map
    x = boundary_map(shape, seed=seed)
    cfg = dict(size_filter=0, apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=1.0)
    return O.ws_blocks(cfg, shape, [dict(input=x)])[0]['output'], x


def ids_below_median(labels):
    ids, counts = np.unique(labels, return_counts=True)
    ids, counts = ids[ids != 0], counts[ids != 0]
    return ids[counts < np.median(counts)].astype(np.uint64)


def apply_block(labels, discard_ids, hmap=None):
    """-> (status, output or None)."""
    labels = np.asarray(labels, dtype=np.uint64)
    if not labels.any():
        return ZERO, None
    discard = np.isin(labels, np.asarray(discard_ids, dtype=np.uint64))
    if not discard.any():
        return COPIED, labels.copy()
    seeds = np.where(discard, np.uint64(0), labels)
    if hmap is None:
        return WRITTEN, seeds
    values, compact = np.unique(seeds, return_inverse=True)
    compact = compact.reshape(seeds.shape)
    if values[0] != 0:  # no background left: compact ids start at 1
        values = np.concatenate([np.zeros(1, np.uint64), values])
        compact = compact + 1
    assert len(values) < 2 ** 32
    ws, _ = O.watershed(np.asarray(hmap).astype(np.float32), compact.astype(np.uint32))
    if len(values) == 1:  # no seed left: vigra's own seeds, output as they are
        return WRITTEN, ws.astype(np.uint64)
    return WRITTEN, values[ws]
