"""CPU tests of the morphology restatement (tests/morphology_ref.py): the
vectorised block table against a triple loop, the merge of the blocks' tables against the whole
volume in exact arithmetic, and the on-disk form through a real n5 variable-length chunk."""
from fractions import Fraction

import numpy as np
import pytest

from cluster_tools_amd.io import File
from cluster_tools_amd.morphology import serialization as S
from cluster_tools_amd.morphology.merge_morphology import merge_rows
from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.utils import volume_utils as vu
import morphology_ref as R


def _tiny(seed, shape):
    rng = np.random.RandomState(seed)
    lab = rng.randint(0, 5, shape).astype(np.uint64)
    lab[lab == 4] = 2 ** 40 + 3
    return lab


@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 3, 4), (5, 6, 7), (1, 6, 1)])
@pytest.mark.parametrize('begin', [(0, 0, 0), (1000, 2 ** 20, 7)])
def test_restatement_equals_the_triple_loop(shape, begin):
    lab = _tiny(sum(shape), shape)
    got, want = R.block_morphology(lab, begin), R.block_morphology_brute(lab, begin)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.float64 and got.shape == (len(np.unique(lab)), 11)
    assert (np.diff(got[:, 0]) > 0).all() and got[:, 1].sum() == lab.size
    # minima and maxima are inclusive and global
    assert (got[:, 5:8] >= np.array(begin)).all()
    assert (got[:, 8:11] <= np.array(begin) + np.array(shape) - 1).all()


def test_a_single_id_fills_the_block():
    got = R.block_morphology(np.full((2, 3, 4), 7, np.uint64), (10, 20, 30))
    assert got.tolist() == [[7, 24, 10.5, 21, 31.5, 10, 20, 30, 11, 22, 33]]


def _volume(seed, shape, cell):
    rng = np.random.RandomState(seed)
    coarse = rng.randint(0, 12, tuple(-(-s // c) for s, c in zip(shape, cell))).astype(np.uint64)
    vol = np.kron(coarse, np.ones(cell, dtype=np.uint64))[tuple(slice(0, s) for s in shape)]
    vol[rng.rand(*shape) < .02] = 13
    return np.ascontiguousarray(vol)


@pytest.mark.parametrize('merge', ['restatement', 'package'])
def test_merged_blocks_equal_the_whole_volume(merge):
    shape, block_shape = (20, 30, 45), [8, 8, 16]
    vol = _volume(3, shape, (5, 7, 9))
    blocking = Blocking([0, 0, 0], list(shape), block_shape)
    assert blocking.numberOfBlocks == 36
    tables, holders = [], {}
    for block_id in range(blocking.numberOfBlocks):
        block = blocking.getBlock(block_id)
        t = R.block_morphology(vol[vu.block_to_bb(block)], block.begin)
        tables.append(t)
        for i in t[:, 0]:
            holders[int(i)] = holders.get(int(i), 0) + 1
    n_labels = 16  # ids 14 and 15 occur nowhere
    if merge == 'restatement':
        got = R.merge_morphology(n_labels, tables)
    else:
        got = merge_rows(np.concatenate(tables), 0, n_labels)
        np.testing.assert_array_equal(got, R.merge_morphology(n_labels, tables))
        np.testing.assert_array_equal(merge_rows(np.concatenate(tables), 3, 9), got[3:9])
    exact = R.volume_exact(vol)
    assert max(holders.values()) > 20
    worst = 0.
    for i in range(n_labels):
        if i not in exact:
            assert not got[i].any()
            continue
        n, com, lo, hi = exact[i]
        assert got[i, 0] == i and got[i, 1] == n
        assert tuple(got[i, 5:8]) == lo and tuple(got[i, 8:11]) == hi
        bound = R.centre_bound(holders[i], shape)
        for a in range(3):
            err = abs(Fraction(float(got[i, 2 + a])) - com[a])
            assert err <= Fraction(bound), (i, a, float(err), bound)
            worst = max(worst, float(err) / bound)
    assert worst < 1.


def test_merge_refuses_an_id_out_of_range():
    t = R.block_morphology(np.array([[[1, 9]]], np.uint64))
    with pytest.raises(RuntimeError, match='id 9'):
        R.merge_morphology(9, [t])
    assert R.merge_morphology(10, [t])[9, 1] == 1


def test_serialization_round_trip(tmp_path):
    rows = R.block_morphology(_tiny(1, (4, 5, 6)), (8, 0, 4))
    flat = S.serialize_morphology(rows)
    assert flat.dtype == np.float64 and flat.shape == (11 * len(rows),)
    np.testing.assert_array_equal(S.deserialize_morphology(flat), rows)
    with pytest.raises(ValueError, match='morphology chunk'):
        S.deserialize_morphology(flat[:-1])
    with pytest.raises(ValueError, match='morphology rows'):
        S.serialize_morphology(rows[:, :10])
    # through a dataset, as the tasks write it
    ds = File(str(tmp_path / 'a.n5')).create_dataset('m', shape=(8, 8, 8), chunks=(4, 4, 4), dtype='float64',
                                                     compression='gzip')
    ds.write_chunk((1, 0, 1), flat, True)
    np.testing.assert_array_equal(ds.read_chunk((1, 0, 1)), flat)
    np.testing.assert_array_equal(S.read_morphology_rows(ds, (1, 0, 1)), rows)
    assert S.read_morphology_rows(ds, (0, 1, 1)).shape == (0, 11)  # a chunk that was not written
    ds.write_chunk((0, 0, 0), np.zeros((4, 4, 4), 'float64'))  # a fixed-size chunk is no table
    with pytest.raises(ValueError, match='variable-length'):
        S.read_morphology_rows(ds, (0, 0, 0))


def test_variable_length_chunks_are_refused_for_zarr(tmp_path):
    ds = File(str(tmp_path / 'a.zarr')).create_dataset('m', shape=(8, 8, 8), chunks=(4, 4, 4), dtype='float64')
    with pytest.raises(NotImplementedError, match='n5'):
        ds.write_chunk((0, 0, 0), np.zeros(11), True)


def test_against_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    lab = _volume(5, (9, 14, 20), (3, 5, 6)).astype(np.int64)
    got = R.block_morphology(lab.astype(np.uint64))
    ids = got[:, 0].astype(np.int64)
    com = np.array(ndimage.center_of_mass(np.ones(lab.shape), lab, ids))
    np.testing.assert_allclose(got[:, 2:5], com, rtol=0, atol=1e-9)
    for row in got[got[:, 0] > 0]:
        sl = ndimage.find_objects(lab)[int(row[0]) - 1]
        assert [s.start for s in sl] == row[5:8].tolist() and [s.stop - 1 for s in sl] == row[8:11].tolist()
