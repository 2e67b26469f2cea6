"""Variable-length n5 chunks (io/chunked.py): `write_chunk(cid, arr, varlen=True)` stores a 1-D
array of any length in n5's chunk mode 1, `read_chunk` returns it, region access over such a chunk
is refused, fixed-size chunks are untouched and zarr datasets refuse the mode."""
import os

import numpy as np
import pytest

from cluster_tools_amd.io import File


@pytest.mark.parametrize('dtype', ['uint64', 'float32'])
@pytest.mark.parametrize('compression', ['gzip', 'raw'])
def test_round_trip(tmp_path, dtype, compression):
    f = File(str(tmp_path / 'a.n5'))
    ds = f.create_dataset('x', shape=(20, 30), chunks=(10, 10), dtype=dtype, compression=compression)
    rng = np.random.RandomState(0)
    data = {(0, 0): np.zeros(0, dtype), (0, 1): np.array([7], dtype),
            (1, 2): (rng.rand(5000) * 2 ** 40).astype(dtype)}
    if dtype == 'uint64':
        data[(1, 2)][:3] = [0, 2 ** 64 - 1, 2 ** 32 + 1]
    for cid, arr in data.items():
        ds.write_chunk(cid, arr, varlen=True)
    ds = File(str(tmp_path / 'a.n5'), 'r')['x']
    for cid, arr in data.items():
        got = ds.read_chunk(cid)
        assert got.dtype == np.dtype(dtype) and got.shape == arr.shape
        np.testing.assert_array_equal(got, arr)
        assert got.dtype.isnative
    assert ds.read_chunk((1, 1)) is None


def test_header_bytes_of_a_raw_chunk(tmp_path):
    f = File(str(tmp_path / 'a.n5'))
    ds = f.create_dataset('x', shape=(5, 6, 7), chunks=(2, 3, 4), dtype='uint64', compression='raw')
    # chunk (2, 0, 1) covers z 4:5, y 0:3, x 4:7: nominal valid dims (1, 3, 3), stored reversed
    ds.write_chunk((2, 0, 1), np.array([1, 2 ** 40 + 3], 'uint64'), varlen=True)
    with open(os.path.join(ds.path, '1', '0', '2'), 'rb') as fh:
        raw = fh.read()
    assert raw == (b'\x00\x01'                  # mode 1: variable length
                   b'\x00\x03'                  # ndim
                   b'\x00\x00\x00\x03' b'\x00\x00\x00\x03' b'\x00\x00\x00\x01'  # dims, reversed
                   b'\x00\x00\x00\x02'          # number of elements
                   b'\x00\x00\x00\x00\x00\x00\x00\x01'
                   b'\x00\x00\x01\x00\x00\x00\x00\x03')
    assert not [n for n in os.listdir(os.path.join(ds.path, '1', '0')) if 'tmp' in n]
    # the same chunk in fixed-size mode: mode 0 and no element count
    ds.write_chunk((2, 0, 1), np.arange(9, dtype='uint64').reshape(1, 3, 3))
    with open(os.path.join(ds.path, '1', '0', '2'), 'rb') as fh:
        raw = fh.read()
    assert raw[:16] == b'\x00\x00\x00\x03' b'\x00\x00\x00\x03' b'\x00\x00\x00\x03' b'\x00\x00\x00\x01'
    assert len(raw) == 16 + 72


def test_fixed_chunks_are_unchanged(tmp_path):
    f = File(str(tmp_path / 'a.n5'))
    ds = f.create_dataset('x', shape=(20, 30), chunks=(10, 10), dtype='uint64')
    a = np.arange(100, dtype='uint64').reshape(10, 10)
    ds.write_chunk((0, 0), a)
    p = os.path.join(ds.path, '0', '0')
    before = open(p, 'rb').read()
    ds.write_chunk((0, 1), np.arange(17, dtype='uint64'), varlen=True)
    ds.write_chunk((1, 0), a + 5)
    assert open(p, 'rb').read() == before
    np.testing.assert_array_equal(ds.read_chunk((0, 0)), a)
    np.testing.assert_array_equal(ds[10:20, 0:10], a + 5)
    np.testing.assert_array_equal(ds[0:10, 0:10], a)
    # region access over the variable-length chunk is refused with a clear error
    with pytest.raises(ValueError, match='variable-length'):
        ds[0:10, 5:15]
    with pytest.raises(ValueError, match='variable-length'):
        ds[0:3, 12:14] = 1
    np.testing.assert_array_equal(ds.read_chunk((0, 1)), np.arange(17, dtype='uint64'))
    # overwritten in fixed-size mode it is an ordinary chunk again
    ds.write_chunk((0, 1), a + 9)
    np.testing.assert_array_equal(ds[0:10, 5:15], np.concatenate([a[:, 5:], (a + 9)[:, :5]], axis=1))


def test_wrong_arrays_are_refused(tmp_path):
    ds = File(str(tmp_path / 'a.n5')).create_dataset('x', shape=(20,), chunks=(10,), dtype='uint64')
    with pytest.raises(ValueError, match='1-D'):
        ds.write_chunk((0,), np.zeros((2, 2), 'uint64'), varlen=True)
    with pytest.raises(ValueError, match='uint64'):
        ds.write_chunk((0,), np.zeros(3, 'float32'), varlen=True)
    assert ds.read_chunk((0,)) is None


def test_zarr_refuses(tmp_path):
    ds = File(str(tmp_path / 'a.zarr')).create_dataset('x', shape=(20,), chunks=(10,), dtype='uint64')
    with pytest.raises(NotImplementedError, match='zarr'):
        ds.write_chunk((0,), np.zeros(3, 'uint64'), varlen=True)
    assert ds.read_chunk((0,)) is None
    ds.write_chunk((0,), np.arange(10, dtype='uint64'))  # fixed-size chunks as before
    np.testing.assert_array_equal(ds[:10], np.arange(10))
