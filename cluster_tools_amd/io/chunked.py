"""N5 and zarr (v2) chunked datasets with a z5py-like API.

The reference reads and writes through z5py (cluster_tools/utils/volume_utils.py:33-43) and
creates the watershed output with require_dataset(..., chunks=block_shape // 2,
compression='gzip', dtype='uint64') (watershed.py:81-84).  z5py is not installed here, so this
module implements the two on-disk formats directly:

* N5: ``attributes.json`` with F-order ``dimensions`` / ``blockSize``; chunk files at
  ``<ds>/<cx>/<cy>/<cz>`` (reversed coordinates) holding a big-endian header (uint16 mode,
  uint16 ndim, uint32 shape[ndim] reversed) and the big-endian chunk data, gzip-compressed
  (edge chunks are stored truncated).
* zarr v2: ``.zarray`` / ``.zattrs`` / ``.zgroup`` JSON; chunk files ``<ds>/i.j.k`` holding the
  full (padded) chunk in C order, gzip- or zlib-compressed or raw.

Chunk (de)compression (libdeflate through ctypes, zlib as the fallback: deflate.py) runs on a
thread pool of ``n_threads`` (both release the GIL).
"""
import json
import os
import threading
from collections import OrderedDict
from concurrent import futures
from itertools import product

import numpy as np

from cluster_tools_amd.io import deflate

_N5_DTYPES = {'uint8': 'uint8', 'uint16': 'uint16', 'uint32': 'uint32', 'uint64': 'uint64',
              'int8': 'int8', 'int16': 'int16', 'int32': 'int32', 'int64': 'int64',
              'float32': 'float32', 'float64': 'float64'}


def _normalize_index(index, shape):
    if not isinstance(index, tuple):
        index = (index,)
    out = []
    for d, sh in enumerate(shape):
        if d < len(index) and index[d] is not Ellipsis:
            ind = index[d]
            if isinstance(ind, slice):
                start, stop, step = ind.indices(sh)
                assert step == 1, "strided access is not supported"
                out.append(slice(start, max(start, stop)))
            else:
                i = int(ind)
                i = i + sh if i < 0 else i
                out.append(slice(i, i + 1))
        else:
            out.append(slice(0, sh))
    squeeze = tuple(d for d in range(min(len(index), len(shape)))
                    if not isinstance(index[d], slice) and index[d] is not Ellipsis)
    return tuple(out), squeeze


def _compress(arr, compression, level=5):
    """The chunk file payload of the C-contiguous array `arr` (bytes)."""
    if compression in ('gzip', 'zlib'):
        return deflate.deflate(arr, compression, level)
    return arr.tobytes()


def _decompress(data, compression, nbytes):
    """The decompressed payload as a uint8 array of `nbytes` (gzip / zlib header detected)."""
    if compression in ('gzip', 'zlib'):
        out = deflate.inflate(data, nbytes)
    else:
        out = np.frombuffer(data, np.uint8)
    if out.size != nbytes:
        raise ValueError("chunk holds %i bytes, expected %i" % (out.size, nbytes))
    return out


def _dump_json(path, obj):
    """Write a metadata / attributes file atomically (temp file + rename): in N5 the attributes
    share attributes.json with the dataset metadata, and jobs open the dataset (reading it) while
    job 0 sets attrs (write.py's maxId) — a truncate-and-rewrite would let them read it empty."""
    tmp = '%s.tmp%d.%d' % (path, os.getpid(), threading.get_ident())
    with open(tmp, 'w') as f:
        json.dump(obj, f)
    os.replace(tmp, path)


class Attributes:
    def __init__(self, path, fmt):
        self._path = path
        self._fmt = fmt

    def _file(self):
        return os.path.join(self._path, 'attributes.json' if self._fmt == 'n5' else '.zattrs')

    def _load(self):
        if os.path.exists(self._file()):
            with open(self._file()) as f:
                return json.load(f)
        return {}

    def __getitem__(self, k):
        return self._load()[k]

    def __setitem__(self, k, v):
        a = self._load()
        a[k] = v
        _dump_json(self._file(), a)

    def __contains__(self, k):
        return k in self._load()

    def get(self, k, default=None):
        return self._load().get(k, default)

    def items(self):
        return self._load().items()


class Dataset:
    def __init__(self, path, fmt):
        self.path = path
        self.fmt = fmt
        self.n_threads = 1
        # decompressed-chunk cache for reads (bytes; 0 = off): blocks read with halos share their
        # border chunks, a job reading neighbouring blocks then inflates each chunk once
        self.cache_bytes = 0
        self._cache = OrderedDict()
        self._cache_used = 0
        self._cache_lock = threading.Lock()
        self._varlen = set()  # ids of the chunks read in n5's variable-length mode
        if fmt == 'n5':
            with open(os.path.join(path, 'attributes.json')) as f:
                meta = json.load(f)
            self.shape = tuple(meta['dimensions'][::-1])
            self.chunks = tuple(meta['blockSize'][::-1])
            self.dtype = np.dtype(meta['dataType'])
            comp = meta.get('compression', {'type': 'raw'})
            self.compression = comp.get('type', 'raw') if isinstance(comp, dict) else 'raw'
            if self.compression == 'gzip' and comp.get('useZlib'):
                self.compression = 'zlib'  # n5 "gzip" with the zlib wrapper
            self._fill = 0
        else:
            with open(os.path.join(path, '.zarray')) as f:
                meta = json.load(f)
            self.shape = tuple(meta['shape'])
            self.chunks = tuple(meta['chunks'])
            self.dtype = np.dtype(meta['dtype'])
            comp = meta.get('compressor')
            self.compression = 'raw' if comp is None else comp['id']
            self._fill = meta.get('fill_value') or 0
            self._sep = meta.get('dimension_separator', '.')
        self.ndim = len(self.shape)
        self.attrs = Attributes(path, fmt)

    @property
    def size(self):
        return int(np.prod(self.shape))

    @property
    def chunks_per_dimension(self):
        return [int(np.ceil(s / float(c))) for s, c in zip(self.shape, self.chunks)]

    @property
    def number_of_chunks(self):
        return int(np.prod(self.chunks_per_dimension))

    # ---- chunk io -------------------------------------------------------------------
    def _chunk_path(self, cid):
        if self.fmt == 'n5':
            return os.path.join(self.path, *[str(c) for c in cid[::-1]])
        return os.path.join(self.path, self._sep.join(str(c) for c in cid))

    def _chunk_bb(self, cid):
        beg = [c * s for c, s in zip(cid, self.chunks)]
        end = [min(b + s, sh) for b, s, sh in zip(beg, self.chunks, self.shape)]
        return beg, end

    def read_chunk(self, cid):
        """Chunk data (valid region, C order) or None if the chunk does not exist."""
        if self.cache_bytes:
            with self._cache_lock:
                hit = self._cache.get(cid)
                if hit is not None:
                    self._cache.move_to_end(cid)
                    return hit
        arr = self._read_chunk(cid)
        if self.cache_bytes and arr is not None and arr.nbytes <= self.cache_bytes:
            with self._cache_lock:
                if cid not in self._cache:
                    self._cache[cid] = arr
                    self._cache_used += arr.nbytes
                    while self._cache_used > self.cache_bytes:
                        _, old = self._cache.popitem(last=False)
                        self._cache_used -= old.nbytes
        return arr

    def _read_chunk(self, cid):
        p = self._chunk_path(cid)
        if not os.path.exists(p):
            return None
        with open(p, 'rb') as f:
            raw = f.read()
        beg, end = self._chunk_bb(cid)
        if self.fmt == 'n5':
            mode, nd = (int(v) for v in np.frombuffer(raw[:4], dtype='>u2'))
            if mode not in (0, 1):
                raise ValueError("n5 chunk %s has mode %i (0: fixed size, 1: variable length)" % (p, mode))
            cshape = tuple(np.frombuffer(raw[4:4 + 4 * nd], dtype='>u4')[::-1].astype(int))
            off = 4 + 4 * nd
            if mode == 1:
                # variable length: the element count follows the nominal dims, the data is 1-D
                cshape = (int(np.frombuffer(raw[off:off + 4], dtype='>u4')[0]),)
                off += 4
                self._varlen.add(tuple(cid))
            else:
                self._varlen.discard(tuple(cid))
            data = _decompress(raw[off:], self.compression,
                               int(np.prod(cshape)) * self.dtype.itemsize)
            arr = data.view(self.dtype.newbyteorder('>')).reshape(cshape)
            if not arr.flags.writeable:
                return arr.astype(self.dtype)
            # big-endian -> native in place (the inflated buffer is ours)
            return arr.byteswap(inplace=True).view(self.dtype)
        data = _decompress(raw, self.compression, int(np.prod(self.chunks)) * self.dtype.itemsize)
        arr = data.view(self.dtype).reshape(self.chunks)
        return arr[tuple(slice(0, e - b) for b, e in zip(beg, end))]

    def write_chunk(self, cid, arr, varlen=False):
        """Write one chunk: `arr` has the chunk's valid shape; with varlen=True (n5 only, z5py's
        `write_chunk(cid, arr, True)`) it is 1-D, of the dataset's dtype and of any length, and the
        chunk is stored in n5's variable-length mode."""
        beg, end = self._chunk_bb(cid)
        valid = tuple(e - b for b, e in zip(beg, end))
        if varlen:
            if self.fmt != 'n5':
                raise NotImplementedError("variable-length chunks exist only in n5 (chunk mode 1); zarr has no "
                                          "portable form for them (a zarr chunk always holds the full chunk shape)")
            arr = np.asarray(arr)
            if arr.ndim != 1 or arr.dtype != self.dtype:
                raise ValueError("a variable-length chunk is 1-D and of dtype %s, not %i-D %s"
                                 % (self.dtype, arr.ndim, arr.dtype))
        else:
            assert arr.shape == valid, (arr.shape, valid)
        p = self._chunk_path(cid)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        if self.fmt == 'n5':
            header = np.array([1 if varlen else 0, len(valid)], dtype='>u2').tobytes() + \
                np.array(valid[::-1], dtype='>u4').tobytes()
            if varlen:
                header += np.array([arr.size], dtype='>u4').tobytes()
            payload = _compress(np.ascontiguousarray(arr, dtype=self.dtype.newbyteorder('>')), self.compression)
            data = header + payload
        else:
            full = np.full(self.chunks, self._fill, dtype=self.dtype)
            full[tuple(slice(0, v) for v in valid)] = arr
            data = _compress(full, self.compression)
        tmp = p + '.tmp%d' % os.getpid()
        with open(tmp, 'wb') as f:
            f.write(data)
        os.replace(tmp, p)

    def _refuse_varlen(self, cid):
        """Region access has no meaning for a variable-length chunk: its data is no box of voxels."""
        if tuple(cid) in self._varlen:
            raise ValueError("chunk %s of %s is a variable-length n5 chunk: it holds a 1-D sequence, not the "
                             "voxels of its region; read it with read_chunk" % (tuple(cid), self.path))

    def _chunk_ids(self, bb):
        ranges = [range(s.start // c, (s.stop - 1) // c + 1) if s.stop > s.start else range(0)
                  for s, c in zip(bb, self.chunks)]
        return list(product(*ranges))

    def _map(self, fn, items):
        if self.n_threads > 1 and len(items) > 1:
            with futures.ThreadPoolExecutor(self.n_threads) as tp:
                return list(tp.map(fn, items))
        return [fn(i) for i in items]

    def __getitem__(self, index):
        return self.read_many([index])[0]

    def read_many(self, indices):
        """[self[i] for i in indices], with the chunks of all of them read and inflated by one
        pool (each chunk once, copied into every array that overlaps it): a batch of blocks
        keeps n_threads busy where a block with few chunks of its own would not."""
        bbs = [_normalize_index(i, self.shape) for i in indices]
        # every voxel is written below: from its chunk, or the fill value where none is stored
        outs = [np.empty(tuple(s.stop - s.start for s in bb), dtype=self.dtype) for bb, _ in bbs]
        users = OrderedDict()
        for k, (bb, _) in enumerate(bbs):
            for cid in self._chunk_ids(bb):
                users.setdefault(cid, []).append(k)

        def load(cid):
            data = self.read_chunk(cid)
            self._refuse_varlen(cid)
            beg, end = self._chunk_bb(cid)
            for k in users[cid]:
                bb = bbs[k][0]
                src, dst = [], []
                for s, b, e in zip(bb, beg, end):
                    lo, hi = max(s.start, b), min(s.stop, e)
                    src.append(slice(lo - b, hi - b))
                    dst.append(slice(lo - s.start, hi - s.start))
                outs[k][tuple(dst)] = self._fill if data is None else data[tuple(src)]

        self._map(load, list(users))
        return [o.squeeze(axis=sq) if sq else o for o, (_, sq) in zip(outs, bbs)]

    def __setitem__(self, index, value):
        bb, _ = _normalize_index(index, self.shape)
        value = np.asarray(value)
        tshape = tuple(s.stop - s.start for s in bb)
        if value.shape != tshape:
            value = np.broadcast_to(value, tshape)

        def store(cid):
            beg, end = self._chunk_bb(cid)
            src, dst, full = [], [], True
            for s, b, e in zip(bb, beg, end):
                lo, hi = max(s.start, b), min(s.stop, e)
                src.append(slice(lo - s.start, hi - s.start))
                dst.append(slice(lo - b, hi - b))
                full &= (lo == b and hi == e)
            if full:
                chunk = np.ascontiguousarray(value[tuple(src)], dtype=self.dtype)
            else:
                old = self._read_chunk(cid)
                self._refuse_varlen(cid)
                chunk = np.full(tuple(e - b for b, e in zip(beg, end)), self._fill, dtype=self.dtype) \
                    if old is None else old.copy()
                chunk[tuple(dst)] = value[tuple(src)]
            self.write_chunk(cid, chunk)

        self._map(store, self._chunk_ids(bb))


class Group:
    def __init__(self, path, fmt, mode='a'):
        self.path = path
        self.fmt = fmt
        self.mode = mode
        self.attrs = Attributes(path, fmt)

    def _is_dataset(self, p):
        return os.path.exists(os.path.join(p, 'attributes.json' if self.fmt == 'n5' else '.zarray')) and \
            (self.fmt != 'n5' or 'dimensions' in json.load(open(os.path.join(p, 'attributes.json'))))

    def __contains__(self, key):
        return os.path.isdir(os.path.join(self.path, key))

    def __getitem__(self, key):
        p = os.path.join(self.path, key)
        if not os.path.isdir(p):
            raise KeyError(key)
        return Dataset(p, self.fmt) if self._is_dataset(p) else Group(p, self.fmt, self.mode)

    def __delitem__(self, key):
        # as h5py's `del f[key]`, so callers can drop a dataset without knowing the layout
        p = os.path.join(self.path, key)
        if not os.path.isdir(p):
            raise KeyError(key)
        import shutil
        shutil.rmtree(p)

    def keys(self):
        return sorted(d for d in os.listdir(self.path) if os.path.isdir(os.path.join(self.path, d)))

    def require_group(self, key):
        p = os.path.join(self.path, key)
        os.makedirs(p, exist_ok=True)
        if self.fmt == 'zarr' and not os.path.exists(os.path.join(p, '.zgroup')):
            _dump_json(os.path.join(p, '.zgroup'), {'zarr_format': 2})
        return Group(p, self.fmt, self.mode)

    create_group = require_group

    def create_dataset(self, key, shape=None, dtype=None, chunks=None, compression='gzip', data=None,
                       fillvalue=0, **kwargs):
        if data is not None:
            shape = data.shape if shape is None else shape
            dtype = data.dtype if dtype is None else dtype
        assert shape is not None and dtype is not None
        dtype = np.dtype(dtype)
        chunks = tuple(int(c) for c in (chunks if chunks is not None else shape))
        chunks = tuple(max(1, min(c, s)) if s > 0 else max(1, c) for c, s in zip(chunks, shape))
        p = os.path.join(self.path, key)
        if os.path.exists(p):
            raise RuntimeError("dataset %s exists" % p)
        parent = os.path.dirname(key)
        if parent:
            self.require_group(parent)
        os.makedirs(p)
        comp = compression if compression in ('gzip', 'zlib', 'raw', None) else 'gzip'
        comp = 'raw' if comp is None else comp
        # measurement hook (bench.py end_to_end): store every new dataset uncompressed, to
        # separate the gzip share of an end-to-end run
        comp = os.environ.get('CTWS_N5_COMPRESSION', comp)
        if self.fmt == 'n5':
            meta = {'dimensions': list(shape)[::-1], 'blockSize': list(chunks)[::-1],
                    'dataType': _N5_DTYPES[dtype.name],
                    'compression': {'type': comp} if comp == 'raw' else
                    {'type': 'gzip', 'level': 5, 'useZlib': comp == 'zlib'}}
            _dump_json(os.path.join(p, 'attributes.json'), meta)
        else:
            meta = {'chunks': list(chunks), 'compressor': None if comp == 'raw' else {'id': comp, 'level': 5},
                    'dtype': dtype.str, 'fill_value': fillvalue, 'filters': None, 'order': 'C',
                    'shape': list(shape), 'zarr_format': 2}
            _dump_json(os.path.join(p, '.zarray'), meta)
        ds = Dataset(p, self.fmt)
        if data is not None:
            ds[...] = data
        return ds

    def require_dataset(self, key, shape, dtype, chunks=None, compression='gzip', **kwargs):
        p = os.path.join(self.path, key)
        if os.path.exists(p):
            ds = Dataset(p, self.fmt)
            assert tuple(ds.shape) == tuple(shape), "shape mismatch %s vs %s" % (ds.shape, shape)
            return ds
        return self.create_dataset(key, shape=shape, dtype=dtype, chunks=chunks, compression=compression, **kwargs)


class File(Group):
    """z5py.File-like container: ``.n5`` -> N5, ``.zr`` / ``.zarr`` -> zarr v2."""

    def __init__(self, path, mode='a', use_zarr_format=None):
        ext = os.path.splitext(path)[1].lower()
        fmt = 'n5' if ext == '.n5' else 'zarr'
        if use_zarr_format is not None:
            fmt = 'zarr' if use_zarr_format else 'n5'
        if not os.path.exists(path):
            if mode == 'r':
                raise OSError("%s does not exist" % path)
            os.makedirs(path)
            if fmt == 'n5':
                _dump_json(os.path.join(path, 'attributes.json'), {'n5': '2.0.0'})
            else:
                _dump_json(os.path.join(path, '.zgroup'), {'zarr_format': 2})
        super().__init__(path, fmt, mode)

    def __enter__(self):
        return self

    def __exit__(self, *args):
        pass

    def close(self):
        pass
