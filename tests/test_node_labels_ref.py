"""The numpy restatement of the node labels (tests/node_labels_ref.py) against plain Python dict
loops on tiny volumes: the overlap rows with and without ignore label, the merge over blocks and
the max overlap with its tie rule."""
import numpy as np
import pytest

import node_labels_ref as R


def _tiny(seed, shape=(3, 4, 5), n_nodes=5, n_labels=4):
    rng = np.random.RandomState(seed)
    return rng.randint(0, n_nodes, shape).astype(np.uint64), rng.randint(0, n_labels, shape).astype(np.uint64)


@pytest.mark.parametrize('ignore_label', [None, 0, 2])
def test_rows_equal_the_dict_loop(ignore_label):
    for seed in range(3):
        nodes, labels = _tiny(seed)
        rows = R.overlap_rows(nodes, labels, ignore_label)
        assert rows.dtype == np.uint64 and rows.shape[1] == 3
        assert R.rows_to_dict(rows) == R.overlap_dict_brute(nodes, labels, ignore_label)
        # sorted by (node, label), no pair twice
        keys = [tuple(r) for r in rows[:, :2].tolist()]
        assert keys == sorted(set(keys))
        want = nodes.size if ignore_label is None else int((labels != ignore_label).sum())
        assert int(rows[:, 2].sum()) == want


def test_signed_labels_wrap_like_astype():
    nodes, labels = _tiny(5)
    signed = labels.astype(np.int32) - 1
    rows = R.overlap_rows(nodes, signed)
    assert R.rows_to_dict(rows) == R.overlap_dict_brute(nodes, signed)
    assert (rows[:, 1] == np.uint64(2 ** 64 - 1)).any()
    assert not (R.overlap_rows(nodes, signed, -1)[:, 1] == np.uint64(2 ** 64 - 1)).any()


def test_merge_over_blocks_equals_the_whole():
    nodes, labels = _tiny(7, shape=(4, 6, 10), n_nodes=6)
    blocks = [np.s_[:2, :, :5], np.s_[:2, :, 5:], np.s_[2:, :, :5], np.s_[2:, :, 5:]]
    for ignore_label in (None, 1):
        merged = R.merge_rows([R.overlap_rows(nodes[bb], labels[bb], ignore_label) for bb in blocks])
        np.testing.assert_array_equal(merged, R.overlap_rows(nodes, labels, ignore_label))
    assert R.merge_rows([]).shape == (0, 3) and R.merge_rows([None, R.EMPTY]).shape == (0, 3)


def test_skipped_blocks():
    nodes, labels = _tiny(8)
    assert R.block_rows(np.zeros_like(nodes), labels) is None
    assert R.block_rows(nodes, np.full_like(labels, 3), 3) is None
    np.testing.assert_array_equal(R.block_rows(nodes, np.full_like(labels, 3), None),
                                  R.overlap_rows(nodes, np.full_like(labels, 3)))
    np.testing.assert_array_equal(R.block_rows(nodes, labels, 3), R.overlap_rows(nodes, labels, 3))


def test_max_overlap_with_a_tie_and_a_covered_node():
    """node 1: labels 5 and 3 tie at 4 voxels (the smaller wins); node 2 lies wholly under the
    ignore label; node 4 does not occur."""
    nodes = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 0], np.uint64).reshape(1, 3, 5)
    labels = np.array([5, 5, 5, 5, 3, 3, 3, 3, 9, 7, 7, 7, 7, 8, 8], np.uint64).reshape(1, 3, 5)
    for ignore_label, want in ((None, [8, 3, 7, 7, 0]), (7, [8, 3, 7, 8, 7]), (0, [8, 3, 7, 7, 0])):
        rows = R.overlap_rows(nodes, labels, ignore_label)
        got = R.max_overlap(rows, 5, ignore_label)
        assert got.dtype == np.uint64 and got.tolist() == want, (ignore_label, got)
        np.testing.assert_array_equal(got, R.max_overlap_brute(R.overlap_dict_brute(nodes, labels, ignore_label), 5,
                                                               ignore_label))
    assert R.max_overlap(R.EMPTY, 3, None).tolist() == [0, 0, 0]


def test_max_overlap_random_against_the_loop():
    for seed in range(4):
        nodes, labels = _tiny(10 + seed, shape=(2, 4, 6), n_nodes=7, n_labels=3)  # small counts: many ties
        for ignore_label in (None, 1):
            rows = R.overlap_rows(nodes, labels, ignore_label)
            np.testing.assert_array_equal(
                R.max_overlap(rows, 8, ignore_label),
                R.max_overlap_brute(R.overlap_dict_brute(nodes, labels, ignore_label), 8, ignore_label))
