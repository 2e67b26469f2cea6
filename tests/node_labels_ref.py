"""CPU restatement of the node labels for the tests (`ndist.computeAndSerializeLabelOverlaps`,
`ndist.mergeAndSerializeOverlaps` in node_labels/block_node_labels.py:130-170 and
merge_node_labels.py; nifty is not available, so this is a restatement):

  overlap_rows   the rows (node, label, count) of two volumes, sorted by (node, label); with an
                 ignore label the voxels whose LABEL equals it are not counted
  block_rows     the same with the two skip rules of `_labels_for_block`: a block whose fragments
                 sum to 0 and a block whose labels are all the ignore label contribute nothing
  merge_rows     the rows of several blocks with the counts of equal (node, label) summed
  max_overlap    per node the label of the largest count; the smallest label among tied ones; a
                 node without a counted voxel gets the ignore label (0 when that is None)
"""
import numpy as np

EMPTY = np.zeros((0, 3), np.uint64)


def _sum_rows(pairs, counts):
    if len(pairs) == 0:
        return EMPTY.copy()
    uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
    sums = np.zeros(len(uniq), np.uint64)
    np.add.at(sums, inv.ravel(), counts.astype(np.uint64))
    return np.concatenate([uniq.astype(np.uint64), sums[:, None]], axis=1)


def overlap_rows(nodes, labels, ignore_label=None):
    """-> (m, 3) uint64; labels of any integer dtype are taken as .astype('uint64')."""
    nodes = np.asarray(nodes)
    assert nodes.dtype == np.uint64 and nodes.shape == np.asarray(labels).shape
    u = nodes.ravel()
    v = np.asarray(labels).astype('uint64').ravel()
    if ignore_label is not None:
        keep = v != np.uint64(int(ignore_label) & 0xFFFFFFFFFFFFFFFF)
        u, v = u[keep], v[keep]
    return _sum_rows(np.stack([u, v], axis=1), np.ones(len(u), np.uint64))


def block_rows(nodes, labels, ignore_label=None):
    """overlap_rows, or None for a block that `_labels_for_block` skips."""
    nodes = np.asarray(nodes)
    if nodes.sum() == 0:
        return None
    labels = np.asarray(labels).astype('uint64')
    if ignore_label is not None and (labels == np.uint64(ignore_label)).all():
        return None
    return overlap_rows(nodes, labels, ignore_label)


def merge_rows(rows_list):
    rows_list = [np.asarray(r, np.uint64).reshape(-1, 3) for r in rows_list if r is not None]
    if not rows_list:
        return EMPTY.copy()
    rows = np.concatenate(rows_list)
    return _sum_rows(rows[:, :2], rows[:, 2])


def max_overlap(rows, n_nodes, ignore_label=None):
    """-> (n_nodes,) uint64.  rows sorted by (node, label) with every node < n_nodes."""
    out = np.full(n_nodes, 0 if ignore_label is None else ignore_label, dtype=np.uint64)
    rows = np.asarray(rows, np.uint64).reshape(-1, 3)
    if len(rows) == 0:
        return out
    # by node ascending, count descending, label ascending: a node's first row wins
    order = np.lexsort((rows[:, 1], np.iinfo(np.uint64).max - rows[:, 2], rows[:, 0]))
    rows = rows[order]
    first = np.ones(len(rows), bool)
    first[1:] = rows[1:, 0] != rows[:-1, 0]
    out[rows[first, 0].astype(np.int64)] = rows[first, 1]
    return out


def rows_to_dict(rows):
    """{node: {label: count}} with Python ints."""
    d = {}
    for n, l, c in np.asarray(rows, np.uint64).reshape(-1, 3).tolist():
        d.setdefault(n, {})[l] = c
    return d


# ---- the plain Python loops the restatement is checked against (tiny volumes only) ------------
def overlap_dict_brute(nodes, labels, ignore_label=None):
    d = {}
    for n, l in zip(np.asarray(nodes).ravel().tolist(), np.asarray(labels).astype('uint64').ravel().tolist()):
        if ignore_label is not None and l == (int(ignore_label) & 0xFFFFFFFFFFFFFFFF):
            continue
        d.setdefault(n, {})
        d[n][l] = d[n].get(l, 0) + 1
    return d


def max_overlap_brute(d, n_nodes, ignore_label=None):
    out = [0 if ignore_label is None else int(ignore_label)] * n_nodes
    for n, ovlp in d.items():
        best = max(ovlp.values())
        out[n] = min(l for l, c in ovlp.items() if c == best)
    return np.array(out, dtype=np.uint64)
