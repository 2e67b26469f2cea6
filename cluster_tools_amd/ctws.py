"""ctypes binding of libctws.so (include/ctws.h) — the MI355X watershed kernels.

This is the product path: there is no CPU fallback.  If the HIP library is missing or no
GPU is visible, every call raises.  Build the library with ``python __graft_entry__.py`` or
``make -C cluster_tools_amd/csrc``.
"""
import ctypes as C
import os
import threading

import numpy as np

from ._abi import CtwsBlock, make_cfg, dtype_code, CTWS_OK, CTWS_BLOCK_FAILED, CTWS_BLOCK_WRITTEN  # noqa: F401
from ._abi import CTWS_BLOCK_ZERO, CTWS_BLOCK_COPIED, CTWS_F64  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# CTWS_LIB: another build of the library (A/B of build variants in one process tree)
LIB_PATH = os.environ.get('CTWS_LIB') or os.path.join(_HERE, 'libctws.so')

_lib = None
_lock = threading.Lock()


def lib():
    """Load libctws.so (raises OSError if it was not built).

    If torch is importable it is imported first: its bundled libamdhip64 then satisfies
    libctws.so's HIP dependency, so the process has ONE HIP runtime and device pointers,
    streams and contexts are shared with torch.
    """
    global _lib
    with _lock:
        if _lib is None:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
            if not os.path.exists(LIB_PATH):
                raise OSError("libctws.so not found at %s: build it with `make -C %s/csrc`"
                              % (LIB_PATH, _HERE))
            L = C.CDLL(LIB_PATH)
            L.ctws_abi_version.restype = C.c_int
            if L.ctws_abi_version() != ABI_VERSION:
                raise OSError("libctws.so ABI version %d, expected %d (include/ctws.h): rebuild it"
                              % (L.ctws_abi_version(), ABI_VERSION))
            for name, (argtypes, restype) in SIGNATURES.items():
                fn = getattr(L, name)
                fn.argtypes, fn.restype = argtypes, restype
            _lib = L
        return _lib


# include/ctws.h CTWS_ABI_VERSION (2: the library's own RCCL communicator entry points removed)
ABI_VERSION = 2

_p, _i, _i64, _u64, _f64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_double
_pi, _pi64 = C.POINTER(C.c_int), C.POINTER(C.c_int64)
_BLOCKS = ((_p, _p, _p, _i), _i)  # handle, cfg, blocks, n_blocks
_RAG = ((_p, _p, _i64, _i64, _i64, _i, _p, _i64, _pi64, _p, _p, _i64, _pi64), _i)
_OVERLAPS = ((_p, _p, _p, _i64, _i, _u64, _p, _i64, _pi64), _i)
_MORPHOLOGY = ((_p, _p, _i64, _i64, _i64, _pi64, _p, _i64, _pi64), _i)
_REGION_FEATURES = ((_p, _p, _p, _i, _i64, _i64, _i64, _i, _u64, _p, _i64, _pi64), _i)
_DOWNSCALE = ((_p, _p, _i, _i64, _i64, _i64, _pi64, _i, _p, _i64, _i64, _i64, _pi), _i)
_IMAGE_FILTER = ((_p, _p, _i, _i64, _i64, _i64, _i, C.POINTER(_f64), _i, _i, _p), _i)
_REGION_CENTERS = ((_p, _p, _i64, _i64, _p, _p, _p, _p, C.POINTER(_f64), _p, _p), _i)
_EDGE_FEATURES = ((_p, _p, _p, _i) + (_i64,) * 6 + (_i, _p, _i64, _p, _i64, _p, _pi64), _i)
_LIFTED = ((_p, _p, _i64, _p, _i64, _i, _i, _u64, _p, _i64, _pi64), _i)
_GRAPH_COMPONENTS = ((_p, _p, _i64, _p, _i64, _p), _i)
_GRAPH_WATERSHED = ((_p, _p, _p, _i64, _p, _i64, _i, _p), _i)

# Every function of include/ctws.h: name -> (argtypes, restype).  lib() sets both from this table,
# and its names are the library's exported symbols (tests/test_abi.py holds them against the header).
SIGNATURES = {
    'ctws_abi_version': ([], _i),
    'ctws_open': ([_i, C.POINTER(_p)], _i),
    'ctws_close': ([_p], None),
    'ctws_last_error': ([_p], C.c_char_p),
    'ctws_last_timings': ([_p, _p, _p, _i], _i),
    'ctws_ws_blocks': _BLOCKS,
    'ctws_ws_blocks_device': _BLOCKS,
    'ctws_ws_from_seeds': _BLOCKS,
    'ctws_ws_from_seeds_device': _BLOCKS,
    'ctws_unique_u64': ([_p, _p, _i64, _i, _p, _i64, _pi64], _i),
    'ctws_unique_counts_u64': ([_p, _p, _i64, _i, _p, _p, _i64, _pi64], _i),
    'ctws_set_table_u64': ([_p, _p, _p, _i64], _i),
    'ctws_lookup_u64': ([_p, _p, _i64, _i, _p, _p, _i64, _pi64], _i),
    'ctws_ufd_find': ([_i64, _p, _i64, _p], _i),
    'ctws_set_discard_u64': ([_p, _p, _i64], _i),
    'ctws_size_filter_blocks': ([_p, _p, _i, _i], _i),
    'ctws_size_filter_blocks_device': ([_p, _p, _i, _i], _i),
    'ctws_unique_pairs_u64': ([_p, _p, _p, _i64, _i, _p, _p, _i64, _pi64], _i),
    'ctws_rag_block': _RAG,
    'ctws_rag_block_device': _RAG,
    'ctws_label_overlaps': _OVERLAPS,
    'ctws_label_overlaps_device': _OVERLAPS,
    'ctws_block_morphology': _MORPHOLOGY,
    'ctws_block_morphology_device': _MORPHOLOGY,
    'ctws_region_features_block': _REGION_FEATURES,
    'ctws_region_features_block_device': _REGION_FEATURES,
    'ctws_downscale_block': _DOWNSCALE,
    'ctws_downscale_block_device': _DOWNSCALE,
    'ctws_filter_taps': ([_f64, _i, _p, _pi], _i),
    'ctws_image_filter': _IMAGE_FILTER,
    'ctws_image_filter_device': _IMAGE_FILTER,
    'ctws_region_centers': _REGION_CENTERS,
    'ctws_region_centers_device': _REGION_CENTERS,
    'ctws_edge_features_block': _EDGE_FEATURES,
    'ctws_edge_features_block_device': _EDGE_FEATURES,
    'ctws_lifted_neighborhood': _LIFTED,
    'ctws_lifted_neighborhood_device': _LIFTED,
    'ctws_lifted_limits': ([_i64, _pi64, _pi64], _i),
    'ctws_graph_components': _GRAPH_COMPONENTS,
    'ctws_graph_components_device': _GRAPH_COMPONENTS,
    'ctws_graph_watershed': _GRAPH_WATERSHED,
    'ctws_graph_watershed_device': _GRAPH_WATERSHED,
    'ctws_threshold_components': ([_p, _p, _p, _i64, _i64, _i64, _i, _i, _f64, _i, _p, _pi64], _i),
    'ctws_threshold_components_ex': ([_p, _p, _i, _p, _i64, _i64, _i64, _i, _i, _f64, _i, _f64, _p, _pi64], _i),
    'ctws_eval_begin': ([_p, _i64, _i64], _i),
    'ctws_eval_add': ([_p, _p, _p, _i64, _i, _i], _i),
    'ctws_eval_end': ([_p, _p, _pi64], _i),
    'ctws_debug_set_stop': ([_p, _i], _i),
    'ctws_debug_read': ([_p, C.c_char_p, _i, _p, _i64], _i),
    'ctws_debug_sqrt_int': ([_p, C.c_uint32, C.c_uint32, _p], _i),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)


def ufd_find(n_labels, pairs):
    """nifty.ufd.boost_ufd(n_labels).merge(pairs); .find(arange(n_labels)) in libctws.so (host
    code, no GPU handle): the representative of every label, uint64."""
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint64).reshape(-1, 2))
    out = np.empty(int(n_labels), dtype=np.uint64)
    ret = lib().ctws_ufd_find(int(n_labels), pairs.ctypes.data if pairs.size else None, len(pairs),
                              out.ctypes.data)
    if ret != CTWS_OK:
        raise CtwsError("ctws_ufd_find failed (%i): labels out of range" % ret)
    return out


class CtwsError(RuntimeError):
    pass


# ImageFilter: the filters the library computes (one float32 value per voxel) and vigra's
# multi-channel ones, which the reference's 3-D float32 output dataset cannot hold either
IMAGE_FILTERS = {'gaussianSmoothing': 0, 'gaussianGradientMagnitude': 1, 'laplacianOfGaussian': 2}
MULTI_CHANNEL_FILTERS = ('gaussianGradient', 'hessianOfGaussian', 'hessianOfGaussianEigenvalues',
                         'structureTensor', 'structureTensorEigenvalues')


def filter_taps(sigma, order):
    """The 2 r + 1 double taps (offsets -r .. r) of the Gaussian (order 0) or its first or second
    derivative as the library's filters use them (include/ctws.h, ctws_filter_taps).  Host code,
    no GPU handle."""
    r = C.c_int(0)
    ret = lib().ctws_filter_taps(float(sigma), int(order), None, C.byref(r))
    if ret != CTWS_OK:
        raise ValueError("filter_taps: sigma is positive and order is 0, 1 or 2, not %r, %r" % (sigma, order))
    out = np.empty(2 * r.value + 1, dtype=np.float64)
    lib().ctws_filter_taps(float(sigma), int(order), out.ctypes.data, C.byref(r))
    return out


def image_filter_check(filter_name, sigma, apply_in_2d=False):
    """The refusals of the image filter, before anything is opened: -> (filter id, the three sigmas
    z, y, x).  NotImplementedError for vigra's multi-channel filters, ValueError for any other
    unknown name, a non-positive sigma or a sigma list together with apply_in_2d (the reference's
    assert)."""
    if filter_name in MULTI_CHANNEL_FILTERS:
        raise NotImplementedError("image filter: %s gives several channels per voxel; only %s are computed"
                                  % (filter_name, ', '.join(IMAGE_FILTERS)))
    if filter_name not in IMAGE_FILTERS:
        raise ValueError("image filter: unknown filter %r (one of %s)" % (filter_name, ', '.join(IMAGE_FILTERS)))
    if isinstance(sigma, (tuple, list)):
        if len(sigma) != 3:
            raise ValueError("image filter: a sigma list has three values (z, y, x), not %r" % (sigma,))
        if apply_in_2d:
            raise ValueError("image filter: a sigma list cannot be combined with apply_in_2d")
        sig = tuple(float(s) for s in sigma)
    else:
        sig = (float(sigma),) * 3
    if not all(s > 0 and np.isfinite(s) for s in sig):
        raise ValueError("image filter: sigma is positive, not %r" % (sigma,))
    return IMAGE_FILTERS[filter_name], sig


# SparseLiftedNeighborhood: the modes of the lifted neighbourhood (include/ctws.h, CTWS_LIFTED_*)
LIFTED_MODES = {'all': 0, 'same': 1, 'different': 2}


def lifted_check(depth, mode):
    """The refusals of the lifted neighbourhood before the call: -> (depth, mode code).  ValueError
    for a depth below 1 (or no integer) and for a mode other than 'all', 'same', 'different'."""
    if mode not in LIFTED_MODES:
        raise ValueError("lifted neighborhood: unknown mode %r (one of %s)" % (mode, ', '.join(LIFTED_MODES)))
    if isinstance(depth, bool) or int(depth) != depth or depth < 1:
        raise ValueError("lifted neighborhood: depth is an integer >= 1, not %r" % (depth,))
    if depth >= 2 ** 31:
        raise ValueError("lifted neighborhood: depth %r does not fit 31 bits" % (depth,))
    return int(depth), LIFTED_MODES[mode]


def lifted_limits(n_sources=0):
    """(first capacity, visited capacity) of the lifted neighbourhood's search (include/ctws.h,
    ctws_lifted_limits): the keys its first pass has room for with n_sources labelled nodes, and
    the nodes a wave's on-chip visited set takes.  Host code, no GPU handle."""
    first, visited = C.c_int64(0), C.c_int64(0)
    ret = lib().ctws_lifted_limits(int(n_sources), C.byref(first), C.byref(visited))
    if ret != CTWS_OK:
        raise ValueError("lifted_limits: n_sources is not negative, not %r" % (n_sources,))
    return int(first.value), int(visited.value)


def _dtype_name(dtype):
    """'uint8', 'float32', ... of a numpy or a torch dtype."""
    return str(dtype).replace('torch.', '')


def _dtype_code(dtype):
    """The library's dtype code of a numpy or a torch dtype."""
    return dtype_code(np.dtype(_dtype_name(dtype)))


class Handle:
    """One library handle = one GPU, one HIP stream, one device workspace."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        ret = lib().ctws_open(int(device), C.byref(self._h))
        if ret != CTWS_OK:
            raise CtwsError("ctws_open(device=%i) failed with %i (no HIP device?)" % (device, ret))
        self.device = device

    def close(self):
        if self._h:
            lib().ctws_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *args):
        self.close()

    def _check(self, ret, what):
        if ret != CTWS_OK:
            msg = lib().ctws_last_error(self._h)
            raise CtwsError("%s failed (%i): %s" % (what, ret, msg.decode() if msg else ''))

    def _call_sized(self, what, caps, call):
        """call(*caps) -> (return code, a size per capacity, the outputs ...), with outputs that
        call allocates (numpy or torch) at the given capacities.  It is called once more, at the
        returned sizes, when the library says that a capacity was too small.  -> (sizes ...,
        outputs ...) of the call that counts; raises as _check."""
        res = call(*caps)
        if res[0] == -1 and any(n > c for n, c in zip(res[1:], caps)):
            res = call(*(max(n, 1) for n in res[1:1 + len(caps)]))
        self._check(res[0], what)
        return res[1:]

    def last_error(self):
        """Message of the last call (also set, with status CTWS_BLOCK_FAILED, for failed blocks)."""
        msg = lib().ctws_last_error(self._h)
        return msg.decode() if msg else ''

    def timings(self):
        n = lib().ctws_last_timings(self._h, None, None, 0)
        names = (C.c_char_p * n)()
        ms = (C.c_float * n)()
        lib().ctws_last_timings(self._h, names, ms, n)
        return {names[i].decode(): float(ms[i]) for i in range(n)}

    # ---- test hooks ----------------------------------------------------------------------
    def debug_set_stop(self, stage):
        self._check(lib().ctws_debug_set_stop(self._h, int(stage)), 'ctws_debug_set_stop')

    def debug_read(self, array, block, shape):
        dt = {'fin': np.float32, 'dt': np.float32, 'seedmap': np.float32, 'hmap': np.float32,
              'labels': np.uint32, 'cls': np.uint8}[array]
        out = np.empty(shape, dtype=dt)
        self._check(lib().ctws_debug_read(self._h, array.encode(), int(block), out.ctypes.data, out.nbytes),
                    'ctws_debug_read')
        return out

    def debug_sqrt_int(self, n0, count):
        """The EDT's integer sqrt (k_edt.hip sqrt_rn_int) of n0 .. n0 + count - 1, as float32."""
        out = np.empty(int(count), dtype=np.float32)
        self._check(lib().ctws_debug_sqrt_int(self._h, int(n0), int(count), out.ctypes.data), 'ctws_debug_sqrt_int')
        return out

    # ---- host (numpy) blocks ------------------------------------------------------------
    def ws_blocks(self, config, block_shape, blocks, pass_id=0):
        """Run `_ws_block` on numpy blocks (see oracle.ws_blocks for the dict layout).

        Returns [{'output': inner uint64, 'status': int, 'max_label': int}, ...].
        """
        cfg = make_cfg(config, block_shape, pass_id)
        n = len(blocks)
        arr = (CtwsBlock * n)()
        keep, results = [], []
        for i, b in enumerate(blocks):
            inp = np.ascontiguousarray(b['input'])
            keep.append(inp)
            c = arr[i]
            c.input = inp.ctypes.data
            c.input_dtype = dtype_code(inp.dtype)
            if inp.ndim == 4:
                c.n_channels = inp.shape[0]
                c.outer_shape[:] = inp.shape[1:]
            else:
                c.n_channels = 0
                c.outer_shape[:] = inp.shape
            oshape = tuple(c.outer_shape)
            if b.get('mask') is not None:
                m = np.ascontiguousarray(b['mask'], dtype=np.uint8)
                keep.append(m)
                c.mask = m.ctypes.data
            c.inner_begin[:] = list(b.get('inner_begin', (0, 0, 0)))
            ishape = tuple(b.get('inner_shape', oshape))
            c.inner_shape[:] = list(ishape)
            c.crop_relabel = int(bool(b.get('crop_relabel', False)))
            c.block_id = int(b.get('block_id', 0))
            if b.get('initial_seeds') is not None:
                s = np.ascontiguousarray(b['initial_seeds'], dtype=np.uint64)
                keep.append(s)
                c.initial_seeds = s.ctypes.data
            out = b.get('out')
            if out is None:
                out = np.empty(ishape, dtype=np.uint64)  # (every voxel of a written block is set)
            assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape == ishape
            keep.append(out)
            c.output = out.ctypes.data
            results.append({'output': out})
        self._check(lib().ctws_ws_blocks(self._h, C.byref(cfg), arr, n), 'ctws_ws_blocks')
        for i, r in enumerate(results):
            r['status'] = int(arr[i].status)
            r['max_label'] = int(arr[i].max_label)
            r['n_ids'] = int(arr[i].n_ids)
        return results

    # ---- device (torch) blocks ----------------------------------------------------------
    def ws_blocks_device(self, config, block_shape, blocks, pass_id=0):
        """Same with torch tensors resident on this GPU: blocks[i] has 'input' (outer tensor),
        'output' (inner uint64/int64 tensor), optional 'mask' (uint8 tensor), 'initial_seeds'
        (outer int64 tensor, pass 2), 'inner_begin', 'crop_relabel', 'block_id'.
        Returns [(status, max_label, n_ids)]."""
        import torch
        cfg = make_cfg(config, block_shape, pass_id)
        n = len(blocks)
        arr = (CtwsBlock * n)()
        # the library runs on its own stream: make torch's pending writes visible first (torch's
        # stream only: other handles' streams on this device keep running)
        torch.cuda.current_stream(blocks[0]['input'].device if blocks else None).synchronize()
        codes = {'torch.uint8': 1, 'torch.uint16': 2, 'torch.float32': 3, 'torch.float64': 4}
        for i, b in enumerate(blocks):
            inp = b['input']
            assert inp.is_contiguous() and inp.is_cuda
            c = arr[i]
            c.input = inp.data_ptr()
            c.input_dtype = codes[str(inp.dtype)]
            if inp.dim() == 4:
                c.n_channels = inp.shape[0]
                c.outer_shape[:] = list(inp.shape[1:])
            else:
                c.n_channels = 0
                c.outer_shape[:] = list(inp.shape)
            if b.get('mask') is not None:
                assert b['mask'].is_contiguous() and b['mask'].element_size() == 1
                c.mask = b['mask'].data_ptr()
            if b.get('initial_seeds') is not None:
                s = b['initial_seeds']
                assert s.is_contiguous() and s.element_size() == 8 and tuple(s.shape) == tuple(c.outer_shape)
                c.initial_seeds = s.data_ptr()
            out = b['output']
            assert out.is_contiguous() and out.element_size() == 8
            c.inner_begin[:] = list(b.get('inner_begin', (0, 0, 0)))
            c.inner_shape[:] = list(out.shape)
            c.crop_relabel = int(bool(b.get('crop_relabel', False)))
            c.block_id = int(b.get('block_id', 0))
            c.output = out.data_ptr()
        self._check(lib().ctws_ws_blocks_device(self._h, C.byref(cfg), arr, n), 'ctws_ws_blocks_device')
        return [(int(arr[i].status), int(arr[i].max_label), int(arr[i].n_ids)) for i in range(n)]

    # ---- WatershedFromSeeds --------------------------------------------------------------
    def ws_from_seeds(self, config, blocks):
        """WatershedFromSeeds `_ws_block[_masked]` (watershed_from_seeds.py:143-199) on numpy
        blocks: dicts with 'input' (block, 3-D or 4-D C,Z,Y,X), 'seeds' (block-shaped ids, as
        ds_seeds[bb] returns them), optional 'mask' and 'out' (uint64, block-shaped).
        Returns [{'output', 'status', 'max_label'}, ...]."""
        cfg = make_cfg(config, (1, 1, 1), 0)
        n = len(blocks)
        arr = (CtwsBlock * n)()
        keep, results = [], []
        for i, b in enumerate(blocks):
            inp = np.ascontiguousarray(b['input'])
            shape = tuple(inp.shape[-3:])
            c = arr[i]
            c.input = inp.ctypes.data
            c.input_dtype = dtype_code(inp.dtype)
            c.n_channels = inp.shape[0] if inp.ndim == 4 else 0
            c.outer_shape[:] = list(shape)
            c.inner_shape[:] = list(shape)
            seeds = np.ascontiguousarray(b['seeds'], dtype=np.uint64)
            assert seeds.shape == shape
            c.initial_seeds = seeds.ctypes.data
            keep += [inp, seeds]
            if b.get('mask') is not None:
                m = np.ascontiguousarray(b['mask'], dtype=np.uint8)
                keep.append(m)
                c.mask = m.ctypes.data
            out = b.get('out')
            if out is None:
                out = np.zeros(shape, dtype=np.uint64)
            assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape == shape
            keep.append(out)
            c.output = out.ctypes.data
            results.append({'output': out})
        self._check(lib().ctws_ws_from_seeds(self._h, C.byref(cfg), arr, n), 'ctws_ws_from_seeds')
        for i, r in enumerate(results):
            r['status'] = int(arr[i].status)
            r['max_label'] = int(arr[i].max_label)
        return results

    # ---- SizeFilterWorkflow ---------------------------------------------------------------
    def set_discard_ids(self, ids):
        """Upload the discard ids (discard_ids.npy of SizeFilterBlocks: ascending, unique) and
        keep them resident on the GPU; an empty list clears the set."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).ravel()
        self._check(lib().ctws_set_discard_u64(self._h, ids.ctypes.data if ids.size else None, ids.size),
                    'ctws_set_discard_u64')

    def size_filter_blocks(self, blocks, fill=False):
        """`apply_block` of BackgroundSizeFilter (fill=False) or FillingSizeFilter (fill=True) on
        numpy blocks: dicts with 'labels' (the block's ids, as ds_in[bb] returns them), 'hmap'
        (the block's raw height map, uint8 / uint16 / float32; fill only) and optional 'out'
        (uint64, block-shaped; may be the labels array itself).  The discard ids are those of
        set_discard_ids.  Returns [{'output', 'status', 'max_label'}, ...]; the output of a block
        with status CTWS_BLOCK_ZERO or CTWS_BLOCK_FAILED is not written."""
        n = len(blocks)
        arr = (CtwsBlock * n)()
        keep, results = [], []
        for i, b in enumerate(blocks):
            labels = np.ascontiguousarray(b['labels'], dtype=np.uint64)
            assert labels.ndim == 3, labels.shape
            shape = labels.shape
            c = arr[i]
            c.initial_seeds = labels.ctypes.data
            c.outer_shape[:] = list(shape)
            c.inner_shape[:] = list(shape)
            c.block_id = int(b.get('block_id', i))
            keep.append(labels)
            if fill:
                hmap = np.ascontiguousarray(b['hmap'])
                assert hmap.shape == shape, (hmap.shape, shape)
                c.input = hmap.ctypes.data
                c.input_dtype = dtype_code(hmap.dtype)
                keep.append(hmap)
            out = b.get('out')
            if out is None:
                out = np.zeros(shape, dtype=np.uint64)
            assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape == shape
            keep.append(out)
            c.output = out.ctypes.data
            results.append({'output': out})
        self._check(lib().ctws_size_filter_blocks(self._h, arr, n, int(bool(fill))), 'ctws_size_filter_blocks')
        for i, r in enumerate(results):
            r['status'] = int(arr[i].status)
            r['max_label'] = int(arr[i].max_label)
        return results

    def size_filter_blocks_device(self, blocks, fill=False):
        """size_filter_blocks on torch tensors on this GPU: 'labels' and 'out' int64 / uint64
        tensors (allocated if 'out' is missing), 'hmap' uint8 / uint16 / float32.  Nothing but the
        per-block facts crosses PCIe.  Returns [{'output', 'status', 'max_label'}, ...]."""
        import torch
        codes = {'torch.uint8': 1, 'torch.uint16': 2, 'torch.float32': 3, 'torch.float64': 4}
        n = len(blocks)
        arr = (CtwsBlock * n)()
        results = []
        for i, b in enumerate(blocks):
            labels = b['labels']
            assert labels.is_cuda and labels.is_contiguous() and labels.element_size() == 8 and labels.dim() == 3
            c = arr[i]
            c.initial_seeds = labels.data_ptr()
            c.outer_shape[:] = list(labels.shape)
            c.inner_shape[:] = list(labels.shape)
            c.block_id = int(b.get('block_id', i))
            if fill:
                hmap = b['hmap']
                assert hmap.is_cuda and hmap.is_contiguous() and tuple(hmap.shape) == tuple(labels.shape)
                c.input = hmap.data_ptr()
                c.input_dtype = codes[str(hmap.dtype)]
            out = b.get('out')
            if out is None:
                out = torch.zeros(labels.shape, dtype=labels.dtype, device=labels.device)
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 8
            assert tuple(out.shape) == tuple(labels.shape)
            c.output = out.data_ptr()
            results.append({'output': out})
        if blocks:
            torch.cuda.current_stream(blocks[0]['labels'].device).synchronize()
        self._check(lib().ctws_size_filter_blocks_device(self._h, arr, n, int(bool(fill))),
                    'ctws_size_filter_blocks_device')
        for i, r in enumerate(results):
            r['status'] = int(arr[i].status)
            r['max_label'] = int(arr[i].max_label)
        return results

    # ---- evaluation (VI / Rand) ---------------------------------------------------------
    def eval_begin(self, cap_labels, cap_pairs):
        """Start a contingency table for at most cap_labels distinct ids per side and
        cap_pairs distinct (gt, seg) pairs."""
        self._check(lib().ctws_eval_begin(self._h, int(cap_labels), int(cap_pairs)), 'ctws_eval_begin')

    def eval_add(self, seg, gt, ignore_gt_zero=False):
        """Add a block: numpy uint64 arrays, or torch tensors (int64 / uint64) on this GPU."""
        on_dev = hasattr(seg, 'data_ptr')
        if on_dev:
            assert seg.is_contiguous() and gt.is_contiguous() and seg.numel() == gt.numel()
            assert seg.element_size() == 8 and gt.element_size() == 8
            import torch
            torch.cuda.current_stream(seg.device).synchronize()
            ps, pg, n = seg.data_ptr(), gt.data_ptr(), seg.numel()
        else:
            seg = np.ascontiguousarray(seg, dtype=np.uint64)
            gt = np.ascontiguousarray(gt, dtype=np.uint64)
            assert seg.size == gt.size
            ps, pg, n = seg.ctypes.data, gt.ctypes.data, seg.size
        self._check(lib().ctws_eval_add(self._h, ps, pg, int(n), int(on_dev), int(bool(ignore_gt_zero))),
                    'ctws_eval_add')

    def eval_end(self):
        """{'vi-split', 'vi-merge', 'adapted-rand-error', 'rand-index', 'n_points'}."""
        sc = (C.c_double * 4)()
        npts = C.c_int64()
        self._check(lib().ctws_eval_end(self._h, sc, C.byref(npts)), 'ctws_eval_end')
        return {'vi-split': sc[0], 'vi-merge': sc[1], 'adapted-rand-error': sc[2], 'rand-index': sc[3],
                'n_points': int(npts.value)}

    def evaluate(self, seg, gt, ignore_gt_zero=False, cap_labels=None, cap_pairs=None):
        """VI / Rand of one segmentation against one groundtruth in a single table.  Without
        capacities the table is sized for the worst case (every voxel its own id), capped."""
        n = int(np.prod(seg.shape))
        cap = min(n, 1 << 26)
        self.eval_begin(cap_labels or cap, cap_pairs or cap)
        self.eval_add(seg, gt, ignore_gt_zero)
        return self.eval_end()

    # ---- RelabelWorkflow kernels ---------------------------------------------------------
    def unique_u64(self, labels):
        """np.unique of a uint64 label array on the GPU (sorted).  numpy in, numpy out."""
        lab = np.ascontiguousarray(labels, dtype=np.uint64).ravel()
        n = C.c_int64(0)
        cap = 1024
        while True:
            out = np.empty(cap, dtype=np.uint64)
            ret = lib().ctws_unique_u64(self._h, lab.ctypes.data, lab.size, 0, out.ctypes.data, cap, C.byref(n))
            if ret == -1 and n.value > cap:
                cap = n.value
                continue
            self._check(ret, 'ctws_unique_u64')
            return out[:n.value]

    def unique_counts_u64(self, labels):
        """np.unique(labels, return_counts=True) on the GPU (radix sort + run-length encoding):
        (sorted uniques uint64, counts uint64)."""
        lab = np.ascontiguousarray(labels, dtype=np.uint64).ravel()
        n = C.c_int64(0)
        cap = 1024
        while True:
            out = np.empty(cap, dtype=np.uint64)
            cnt = np.empty(cap, dtype=np.uint64)
            ret = lib().ctws_unique_counts_u64(self._h, lab.ctypes.data, lab.size, 0, out.ctypes.data,
                                               cnt.ctypes.data, cap, C.byref(n))
            if ret == -1 and n.value > cap:
                cap = n.value
                continue
            self._check(ret, 'ctws_unique_counts_u64')
            return out[:n.value], cnt[:n.value]

    def set_table_u64(self, keys, values):
        """Upload an assignment table (keys ascending) and keep it resident on the GPU."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        values = np.ascontiguousarray(values, dtype=np.uint64)
        assert keys.shape == values.shape and keys.ndim == 1
        self._check(lib().ctws_set_table_u64(self._h, keys.ctypes.data, values.ctypes.data, keys.size),
                    'ctws_set_table_u64')

    def lookup_u64(self, labels, keys=None, values=None):
        """takeDict: labels (uint64 ndarray, modified in place) through the table keys -> values
        (keys ascending; None: the resident table).  Returns the number of labels absent from
        the table (they are left unchanged)."""
        assert labels.dtype == np.uint64 and labels.flags.c_contiguous
        kp = vp = None
        nt = 0
        if keys is not None:
            keys = np.ascontiguousarray(keys, dtype=np.uint64)
            values = np.ascontiguousarray(values, dtype=np.uint64)
            kp, vp, nt = keys.ctypes.data, values.ctypes.data, keys.size
        miss = C.c_int64(0)
        self._check(lib().ctws_lookup_u64(self._h, labels.ctypes.data, labels.size, 0, kp, vp, nt, C.byref(miss)),
                    'ctws_lookup_u64')
        return int(miss.value)

    # ---- ThresholdedComponentsWorkflow kernels --------------------------------------------
    THRESHOLD_MODES = ('greater', 'less', 'equal')

    def threshold_components(self, block, threshold, mode='greater', mask=None, normalize=True, sigma=0.):
        """BlockComponents of one 3-D block on the GPU (block_components.py:143-230): members =
        block `mode` threshold inside the mask, their 26-connected components numbered 1.. in
        C-order of first appearance (skimage.morphology.label).  `block` is the dataset's values
        in its own dtype (float32 / float64 / any 8-64 bit integer): normalize = vu.normalize
        first (float32); sigma > 0 = vu.normalize(gaussianSmoothing(float32 x, sigma)); raw
        values are compared as numpy compares them with a Python float (include/ctws.h
        ctws_threshold_components_ex).  -> (uint64 labels, n_labels); n_labels 0 = no member
        (the labels are then all 0)."""
        from ._abi import TC_DTYPE_CODES
        block = np.ascontiguousarray(block)
        if block.dtype not in TC_DTYPE_CODES:
            raise ValueError("threshold_components: unsupported dtype %s" % block.dtype)
        assert block.ndim == 3, block.shape
        if mode not in self.THRESHOLD_MODES:
            raise RuntimeError("Thresholding Mode %s not supported" % mode)
        mp = None
        if mask is not None:
            mask = np.ascontiguousarray(mask).astype(np.bool_, copy=False).view(np.uint8)
            assert mask.shape == block.shape, (mask.shape, block.shape)
            mp = mask.ctypes.data
        out = np.zeros(block.shape, dtype=np.uint64)
        n = C.c_int64(0)
        self._check(lib().ctws_threshold_components_ex(self._h, block.ctypes.data, TC_DTYPE_CODES[block.dtype], mp,
                                                       *block.shape, 0, self.THRESHOLD_MODES.index(mode),
                                                       float(threshold), 1 if normalize else 0, float(sigma),
                                                       out.ctypes.data, C.byref(n)),
                    'ctws_threshold_components_ex')
        return out, int(n.value)

    def threshold_components_device(self, block, threshold, mode='greater', mask=None, normalize=True, out=None):
        """threshold_components on torch tensors on this GPU: block float32 (Z, Y, X), mask uint8
        or None, out int64 (uint64 bits; allocated if None) -> (out, n_labels).  Nothing crosses
        PCIe but the member flag and the label count; out is left unwritten when n_labels is 0."""
        import torch
        assert block.is_cuda and block.is_contiguous() and block.dtype == torch.float32 and block.dim() == 3
        if mode not in self.THRESHOLD_MODES:
            raise RuntimeError("Thresholding Mode %s not supported" % mode)
        if out is None:
            out = torch.empty(block.shape, dtype=torch.int64, device=block.device)
        assert out.is_contiguous() and out.element_size() == 8 and tuple(out.shape) == tuple(block.shape)
        mp = None
        if mask is not None:
            assert mask.is_cuda and mask.is_contiguous() and mask.dtype == torch.uint8
            assert tuple(mask.shape) == tuple(block.shape)
            mp = mask.data_ptr()
        torch.cuda.current_stream(block.device).synchronize()
        n = C.c_int64(0)
        self._check(lib().ctws_threshold_components(self._h, block.data_ptr(), mp, *block.shape, 1,
                                                    self.THRESHOLD_MODES.index(mode), float(threshold),
                                                    1 if normalize else 0, out.data_ptr(), C.byref(n)),
                    'ctws_threshold_components')
        return out, int(n.value)

    def unique_u64_device(self, labels):
        """np.unique of a uint64 (or int64) torch tensor on this GPU: the sorted uniques as a
        numpy uint64 array (the labels stay in HBM; only the uniques cross PCIe)."""
        import torch
        assert labels.is_cuda and labels.is_contiguous() and labels.element_size() == 8
        torch.cuda.current_stream(labels.device).synchronize()
        n = C.c_int64(0)
        cap = 1024
        while True:
            out = torch.empty(cap, dtype=torch.int64, device=labels.device)
            ret = lib().ctws_unique_u64(self._h, labels.data_ptr(), labels.numel(), 1, out.data_ptr(), cap,
                                        C.byref(n))
            if ret == -1 and n.value > cap:
                cap = n.value
                continue
            self._check(ret, 'ctws_unique_u64')
            return out[:n.value].cpu().numpy().view(np.uint64)

    def lookup_u64_device(self, labels, keys, values):
        """lookup_u64 on a uint64 / int64 torch tensor on this GPU (in place) with a numpy
        table; returns the number of labels absent from it."""
        import torch
        assert labels.is_cuda and labels.is_contiguous() and labels.element_size() == 8
        kd = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64)).to(labels.device)
        vd = torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).view(np.int64)).to(labels.device)
        torch.cuda.current_stream(labels.device).synchronize()
        miss = C.c_int64(0)
        self._check(lib().ctws_lookup_u64(self._h, labels.data_ptr(), labels.numel(), 1, kd.data_ptr(), vd.data_ptr(),
                                          kd.numel(), C.byref(miss)), 'ctws_lookup_u64')
        return int(miss.value)

    # ---- GraphWorkflow kernels ------------------------------------------------------------
    def unique_pairs_u64_raw(self, pairs, weights, cap):
        """One ctws_unique_pairs_u64 call with an output of `cap` rows:
        (return code, n_unique, out (cap, 2), counts (cap,))."""
        pairs = np.ascontiguousarray(pairs, dtype=np.uint64).reshape(-1, 2)
        wp = None
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.uint64).ravel()
            assert weights.size == len(pairs), (weights.size, len(pairs))
            wp = weights.ctypes.data if weights.size else None
        out = np.empty((cap, 2), dtype=np.uint64)
        cnt = np.empty(cap, dtype=np.uint64)
        n = C.c_int64(0)
        ret = lib().ctws_unique_pairs_u64(self._h, pairs.ctypes.data if len(pairs) else None, wp, len(pairs), 0,
                                          out.ctypes.data if cap else None, cnt.ctypes.data if cap else None,
                                          cap, C.byref(n))
        return ret, int(n.value), out, cnt

    def unique_pairs_u64(self, pairs, weights=None):
        """np.unique(pairs, axis=0) of an (n, 2) uint64 array on the GPU with the summed weights of
        equal rows (weights None: their number): (unique rows (m, 2), sums (m,)), both uint64.  The
        edge merge of MergeSubGraphs.  A call that hits the capacity is repeated once with the
        returned size."""
        n_pairs = int(np.asarray(pairs).size // 2)
        m, out, cnt = self._call_sized('ctws_unique_pairs_u64', (min(n_pairs, 4096),),
                                       lambda cap: self.unique_pairs_u64_raw(pairs, weights, cap))
        return out[:m], cnt[:m]

    # first capacities of rag_block (nodes, edges): a 64 x 512 x 512 block of fragments has ~2,700
    # nodes and ~16,500 edges, and a call that does not fit computes everything again
    RAG_CAPS = (1 << 16, 1 << 18)

    def rag_block_raw(self, labels, ignore_label, cap_nodes, cap_edges):
        """One ctws_rag_block call with outputs of the given capacities: (return code, n_nodes,
        n_edges, nodes (cap_nodes,), edges (cap_edges, 2), counts (cap_edges,))."""
        labels = np.ascontiguousarray(labels, dtype=np.uint64)
        assert labels.ndim == 3 and labels.size, labels.shape
        nodes = np.empty(cap_nodes, dtype=np.uint64)
        edges = np.empty((cap_edges, 2), dtype=np.uint64)
        counts = np.empty(cap_edges, dtype=np.uint64)
        nn, ne = C.c_int64(0), C.c_int64(0)
        ret = lib().ctws_rag_block(self._h, labels.ctypes.data, *labels.shape, int(bool(ignore_label)),
                                   nodes.ctypes.data if cap_nodes else None, cap_nodes, C.byref(nn),
                                   edges.ctypes.data if cap_edges else None,
                                   counts.ctypes.data if cap_edges else None, cap_edges, C.byref(ne))
        return ret, int(nn.value), int(ne.value), nodes, edges, counts

    def rag_block(self, labels, ignore_label=True):
        """The region adjacency graph of a 3-D uint64 label block (the extended box of
        InitialSubGraphs): (nodes (n,), edges (m, 2), counts (m,)), uint64.  nodes = np.unique
        (without 0 under ignore_label); edges = the sorted (min, max) id pairs of face-adjacent
        voxels with different ids (none with a 0 under ignore_label); counts = the voxel pairs per
        edge.  A call that hits a capacity is repeated once with the returned sizes."""
        nn, ne, nodes, edges, counts = self._call_sized(
            'ctws_rag_block', self.RAG_CAPS, lambda cn, ce: self.rag_block_raw(labels, ignore_label, cn, ce))
        return nodes[:nn], edges[:ne], counts[:ne]

    def rag_block_device(self, labels, ignore_label=True):
        """rag_block on a uint64 / int64 torch tensor on this GPU; nodes, edges and counts come
        back as int64 tensors (uint64 bits) on the same device: only the two sizes cross PCIe."""
        import torch
        assert labels.is_cuda and labels.is_contiguous() and labels.element_size() == 8 and labels.dim() == 3
        assert labels.numel() > 0
        torch.cuda.current_stream(labels.device).synchronize()
        nn, ne = C.c_int64(0), C.c_int64(0)

        def call(cn, ce):
            nodes = torch.empty(cn, dtype=torch.int64, device=labels.device)
            edges = torch.empty((ce, 2), dtype=torch.int64, device=labels.device)
            counts = torch.empty(ce, dtype=torch.int64, device=labels.device)
            ret = lib().ctws_rag_block_device(self._h, labels.data_ptr(), *labels.shape, int(bool(ignore_label)),
                                              nodes.data_ptr(), cn, C.byref(nn), edges.data_ptr(),
                                              counts.data_ptr(), ce, C.byref(ne))
            return ret, nn.value, ne.value, nodes, edges, counts
        n, m, nodes, edges, counts = self._call_sized('ctws_rag_block_device', self.RAG_CAPS, call)
        return nodes[:n], edges[:m], counts[:m]

    # ---- EdgeFeaturesWorkflow kernels ------------------------------------------------------
    def edge_features_block(self, labels, data, nodes, edges, ignore_label=True, core_shape=None):
        """The boundary-map features of the edges of one block (include/ctws.h,
        ctws_edge_features_block): labels (uint64) and data (float32, or uint8 taken as v / 255) on
        the block's extended box, nodes / edges its sub-graph (Handle.rag_block), core_shape the
        extent of the block itself (None: the whole box).  -> (features (m, 10) float64: mean,
        variance, min, q10, q25, q50, q75, q90, max, count per edge; n_missing = the owned voxel
        pairs whose edge is not in `edges`).  No edges: an empty table without a launch."""
        labels = np.ascontiguousarray(labels, dtype=np.uint64)
        data = np.ascontiguousarray(data)
        nodes = np.ascontiguousarray(nodes, dtype=np.uint64).ravel()
        edges = np.ascontiguousarray(edges, dtype=np.uint64).reshape(-1, 2)
        if labels.ndim != 3 or data.shape != labels.shape or not labels.size:
            raise ValueError("edge features: labels and data are 3-D and of one shape, not %s and %s"
                             % (labels.shape, data.shape))
        if data.dtype not in (np.dtype('float32'), np.dtype('uint8')):
            raise TypeError("edge features: the boundary map is float32 or uint8, not %s" % data.dtype)
        core = self._core_shape(core_shape, labels.shape)
        out = np.zeros((len(edges), 10), dtype=np.float64)
        if len(edges) == 0:
            return out, 0
        miss = C.c_int64(0)
        self._check(lib().ctws_edge_features_block(self._h, labels.ctypes.data, data.ctypes.data, dtype_code(data.dtype),
                                                   *labels.shape, *core, int(bool(ignore_label)), nodes.ctypes.data,
                                                   len(nodes), edges.ctypes.data, len(edges), out.ctypes.data,
                                                   C.byref(miss)), 'ctws_edge_features_block')
        return out, int(miss.value)

    @staticmethod
    def _core_shape(core_shape, shape):
        core = tuple(int(c) for c in (shape if core_shape is None else core_shape))
        if len(core) != 3 or any(c <= 0 or c > s for c, s in zip(core, shape)):
            raise ValueError("edge features: core shape %s does not fit the box %s" % (core, tuple(shape)))
        return core

    def edge_features_block_device(self, labels, data, nodes, edges, ignore_label=True, core_shape=None):
        """edge_features_block on torch tensors on this GPU: labels, nodes and edges uint64 / int64,
        data float32 or uint8; the features come back as a float64 tensor on the same device, only
        n_missing crosses PCIe."""
        import torch
        for t in (labels, data, nodes, edges):
            assert t.is_cuda and t.is_contiguous()
        assert labels.dim() == 3 and labels.numel() > 0 and data.shape == labels.shape
        assert labels.element_size() == 8 and nodes.element_size() == 8 and edges.element_size() == 8
        if data.dtype not in (torch.float32, torch.uint8):
            raise TypeError("edge features: the boundary map is float32 or uint8, not %s" % data.dtype)
        core = self._core_shape(core_shape, tuple(labels.shape))
        m = edges.numel() // 2
        out = torch.zeros((m, 10), dtype=torch.float64, device=labels.device)
        if m == 0:
            return out, 0
        torch.cuda.current_stream(labels.device).synchronize()
        miss = C.c_int64(0)
        self._check(lib().ctws_edge_features_block_device(self._h, labels.data_ptr(), data.data_ptr(),
                                                          _dtype_code(data.dtype), *labels.shape, *core,
                                                          int(bool(ignore_label)), nodes.data_ptr(), nodes.numel(),
                                                          edges.data_ptr(), m, out.data_ptr(), C.byref(miss)),
                    'ctws_edge_features_block_device')
        return out, int(miss.value)

    # ---- LiftedFeaturesFromNodeLabelsWorkflow kernels ---------------------------------------
    # The first capacity of lifted_neighborhood in rows is the library's own first capacity for its
    # keys, 64 per labelled node (lifted_limits): a call that does not fit computes everything again

    def lifted_neighborhood_raw(self, edges, node_labels, depth, mode, ignore_label, cap):
        """One ctws_lifted_neighborhood call with an output of `cap` rows: (return code, n_out,
        out (cap, 2)).  depth and mode as the C call takes them."""
        edges = np.ascontiguousarray(edges, dtype=np.uint64).reshape(-1, 2)
        node_labels = np.ascontiguousarray(node_labels, dtype=np.uint64).ravel()
        out = np.empty((cap, 2), dtype=np.uint64)
        n = C.c_int64(0)
        ret = lib().ctws_lifted_neighborhood(self._h, edges.ctypes.data if len(edges) else None, len(edges),
                                             node_labels.ctypes.data if node_labels.size else None,
                                             node_labels.size, depth, mode, int(ignore_label) & 0xFFFFFFFFFFFFFFFF,
                                             out.ctypes.data if cap else None, cap, C.byref(n))
        return ret, int(n.value), out

    def lifted_neighborhood(self, edges, node_labels, depth, mode='all', ignore_label=0):
        """The lifted edges of a graph under a node labelling (include/ctws.h,
        ctws_lifted_neighborhood): edges (m, 2) uint64 is the merged graph's edge table (u < v, rows
        sorted, unique), node_labels (n,) uint64 is indexed by node id.  -> (k, 2) uint64, sorted:
        the pairs u < v of nodes whose labels both differ from ignore_label, at hop distance
        2 .. depth in the whole graph, with equal labels (mode 'same'), unequal labels
        ('different') or either ('all').  ValueError for a bad depth or mode before the call.  A
        call that hits the capacity is repeated once with the returned size."""
        depth, code = lifted_check(depth, mode)
        node_labels = np.ascontiguousarray(node_labels, dtype=np.uint64).ravel()
        n_sources = int(np.count_nonzero(node_labels != np.uint64(int(ignore_label) & 0xFFFFFFFFFFFFFFFF)))
        k, out = self._call_sized(
            'ctws_lifted_neighborhood', (lifted_limits(n_sources)[0],),
            lambda cap: self.lifted_neighborhood_raw(edges, node_labels, depth, code, ignore_label, cap))
        return out[:k]

    def lifted_neighborhood_device(self, edges, node_labels, depth, mode='all', ignore_label=0):
        """lifted_neighborhood on two uint64 / int64 torch tensors on this GPU; the rows come back
        as an int64 tensor (uint64 bits) on the same device: only their number crosses PCIe."""
        import torch
        depth, code = lifted_check(depth, mode)
        for t in (edges, node_labels):
            assert t.is_cuda and t.is_contiguous() and t.element_size() == 8 and not t.is_floating_point()
        assert edges.numel() % 2 == 0, edges.shape
        torch.cuda.current_stream(edges.device).synchronize()
        n = C.c_int64(0)
        m = edges.numel() // 2
        ignore = int(ignore_label) & 0xFFFFFFFFFFFFFFFF
        signed = ignore - (1 << 64) if ignore >= 1 << 63 and node_labels.dtype == torch.int64 else ignore
        n_sources = int((node_labels != signed).sum().item()) if node_labels.numel() else 0

        def call(cap):
            out = torch.empty((cap, 2), dtype=torch.int64, device=edges.device)
            ret = lib().ctws_lifted_neighborhood_device(
                self._h, edges.data_ptr() if m else None, m, node_labels.data_ptr() if node_labels.numel() else None,
                node_labels.numel(), depth, code, ignore, out.data_ptr(), cap, C.byref(n))
            return ret, n.value, out
        k, out = self._call_sized('ctws_lifted_neighborhood_device', (lifted_limits(n_sources)[0],), call)
        return out[:k]

    # ---- graph postprocessing kernels (ConnectedComponentsWorkflow, SizeFilterAndGraphWatershedWorkflow) ----

    def graph_components(self, edges, assignments):
        """The components of a node labelling in a graph (include/ctws.h, ctws_graph_components):
        edges (m, 2) uint64 holds node ids below n = len(assignments); two nodes are joined when an
        edge connects them and both carry the same non-zero assignment.  -> (n,) uint64: 0 where the
        assignment is 0, else the component's number, from 1 in the order of the components'
        smallest node ids.  CtwsError for an id >= n."""
        edges = np.ascontiguousarray(edges, dtype=np.uint64).reshape(-1, 2)
        assignments = np.ascontiguousarray(assignments, dtype=np.uint64).ravel()
        out = np.empty(assignments.size, dtype=np.uint64)
        self._check(lib().ctws_graph_components(self._h, edges.ctypes.data if len(edges) else None, len(edges),
                                                assignments.ctypes.data if out.size else None, out.size,
                                                out.ctypes.data if out.size else None), 'ctws_graph_components')
        return out

    def graph_components_device(self, edges, assignments):
        """graph_components on two uint64 / int64 torch tensors on this GPU; the result is an int64
        tensor (uint64 bits) on the same device: nothing crosses PCIe."""
        import torch
        for t in (edges, assignments):
            assert t.is_cuda and t.is_contiguous() and t.element_size() == 8 and not t.is_floating_point()
        assert edges.numel() % 2 == 0, edges.shape
        torch.cuda.current_stream(assignments.device).synchronize()
        m, n = edges.numel() // 2, assignments.numel()
        out = torch.empty(n, dtype=torch.int64, device=assignments.device)
        self._check(lib().ctws_graph_components_device(self._h, edges.data_ptr() if m else None, m,
                                                       assignments.data_ptr() if n else None, n,
                                                       out.data_ptr() if n else None), 'ctws_graph_components_device')
        return out

    def graph_watershed(self, edges, weights, seeds, relabel=False):
        """The seeded watershed on a graph (include/ctws.h, ctws_graph_watershed): edges (m, 2)
        uint64 with node ids below n = len(seeds), weights (m,) float64 (float32 is taken as
        float64), seeds (n,) uint64 with 0 for an unlabelled node.  -> (n,) uint64, the labels of
        the sequential flood that pops the edge with the smallest (weight, row index); nodes that
        no seed reaches keep 0.  relabel: renumbered by first appearance over the node index, from
        1, zeros kept.  ValueError for a weight table of another length, CtwsError for an id >= n
        or a NaN weight.  The rounds it took are in timings()['gw_rounds']."""
        edges = np.ascontiguousarray(edges, dtype=np.uint64).reshape(-1, 2)
        weights = np.ascontiguousarray(weights, dtype=np.float64).ravel()
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64).ravel()
        if len(weights) != len(edges):
            raise ValueError("graph watershed: %i weights for %i edges" % (len(weights), len(edges)))
        out = np.empty(seeds.size, dtype=np.uint64)
        m = len(edges)
        self._check(lib().ctws_graph_watershed(self._h, edges.ctypes.data if m else None,
                                               weights.ctypes.data if m else None, m,
                                               seeds.ctypes.data if out.size else None, out.size, int(bool(relabel)),
                                               out.ctypes.data if out.size else None), 'ctws_graph_watershed')
        return out

    def graph_watershed_device(self, edges, weights, seeds, relabel=False):
        """graph_watershed on torch tensors on this GPU: edges and seeds uint64 / int64, weights
        float64 or float32 (converted on the device); the result is an int64 tensor (uint64 bits)
        on the same device."""
        import torch
        for t in (edges, seeds):
            assert t.is_cuda and t.is_contiguous() and t.element_size() == 8 and not t.is_floating_point()
        assert weights.is_cuda and weights.dtype in (torch.float32, torch.float64), weights.dtype
        assert edges.numel() % 2 == 0, edges.shape
        m, n = edges.numel() // 2, seeds.numel()
        if weights.numel() != m:
            raise ValueError("graph watershed: %i weights for %i edges" % (weights.numel(), m))
        weights = weights.to(torch.float64).contiguous().view(-1)
        torch.cuda.current_stream(seeds.device).synchronize()
        out = torch.empty(n, dtype=torch.int64, device=seeds.device)
        self._check(lib().ctws_graph_watershed_device(self._h, edges.data_ptr() if m else None,
                                                      weights.data_ptr() if m else None, m,
                                                      seeds.data_ptr() if n else None, n, int(bool(relabel)),
                                                      out.data_ptr() if n else None), 'ctws_graph_watershed_device')
        return out

    # ---- NodeLabelWorkflow kernels ---------------------------------------------------------
    # first capacity of label_overlaps in rows: a call that does not fit computes everything again
    OVERLAP_CAP = 1 << 18

    @staticmethod
    def _ignore_args(ignore_label):
        """(with_ignore, ignore_label as uint64) of the C call; a negative label wraps as .astype does"""
        if ignore_label is None:
            return 0, 0
        return 1, int(ignore_label) & 0xFFFFFFFFFFFFFFFF

    def label_overlaps_raw(self, nodes_vol, labels_vol, ignore_label, cap):
        """One ctws_label_overlaps call with an output of `cap` rows: (return code, n_rows,
        rows (cap, 3)).  nodes_vol and labels_vol are uint64 arrays of one size."""
        nodes_vol = np.ascontiguousarray(nodes_vol, dtype=np.uint64)
        labels_vol = np.ascontiguousarray(labels_vol, dtype=np.uint64)
        assert nodes_vol.size == labels_vol.size, (nodes_vol.shape, labels_vol.shape)
        rows = np.empty((cap, 3), dtype=np.uint64)
        n = C.c_int64(0)
        wi, il = self._ignore_args(ignore_label)
        size = nodes_vol.size
        ret = lib().ctws_label_overlaps(self._h, nodes_vol.ctypes.data if size else None,
                                        labels_vol.ctypes.data if size else None, size, wi, il,
                                        rows.ctypes.data if cap else None, cap, C.byref(n))
        return ret, int(n.value), rows

    def label_overlaps(self, nodes_vol, labels_vol, ignore_label=None):
        """The overlaps of the fragments nodes_vol (uint64) with a second label volume of the same
        shape (include/ctws.h, ctws_label_overlaps): rows (m, 3) uint64 of (node, label, count),
        sorted by (node, label), count = the voxels with that pair.  labels_vol of any integer dtype
        is taken as .astype('uint64'), as the reference does.  ignore_label not None: voxels whose
        label equals it are not counted.  A call that hits the capacity is repeated once with the
        returned size."""
        nodes_vol = np.asarray(nodes_vol)
        labels_vol = np.asarray(labels_vol)
        if nodes_vol.dtype != np.dtype('uint64'):
            raise TypeError("label overlaps: the fragments are uint64, not %s" % nodes_vol.dtype)
        if labels_vol.dtype.kind not in 'iu':
            raise TypeError("label overlaps: the labels are integers, not %s" % labels_vol.dtype)
        if nodes_vol.shape != labels_vol.shape:
            raise ValueError("label overlaps: fragments and labels are of one shape, not %s and %s"
                             % (nodes_vol.shape, labels_vol.shape))
        labels_vol = labels_vol.astype('uint64', copy=False)
        m, rows = self._call_sized('ctws_label_overlaps', (self.OVERLAP_CAP,),
                                   lambda cap: self.label_overlaps_raw(nodes_vol, labels_vol, ignore_label, cap))
        return rows[:m]

    def label_overlaps_device(self, nodes_vol, labels_vol, ignore_label=None):
        """label_overlaps on two uint64 / int64 torch tensors of one size on this GPU; the rows come
        back as an int64 tensor (uint64 bits) on the same device: only their number crosses PCIe."""
        import torch
        for t in (nodes_vol, labels_vol):
            assert t.is_cuda and t.is_contiguous() and t.element_size() == 8 and not t.is_floating_point()
        assert nodes_vol.numel() == labels_vol.numel(), (nodes_vol.shape, labels_vol.shape)
        torch.cuda.current_stream(nodes_vol.device).synchronize()
        wi, il = self._ignore_args(ignore_label)
        n = C.c_int64(0)

        def call(cap):
            rows = torch.empty((cap, 3), dtype=torch.int64, device=nodes_vol.device)
            ret = lib().ctws_label_overlaps_device(self._h, nodes_vol.data_ptr(), labels_vol.data_ptr(),
                                                   nodes_vol.numel(), wi, il, rows.data_ptr(), cap, C.byref(n))
            return ret, n.value, rows
        m, rows = self._call_sized('ctws_label_overlaps_device', (self.OVERLAP_CAP,), call)
        return rows[:m]

    # ---- MorphologyWorkflow kernels --------------------------------------------------------
    # first capacity of block_morphology in rows: a call that does not fit computes everything again
    MORPHOLOGY_CAP = 1 << 16

    @staticmethod
    def _begin_arg(begin):
        begin = [int(b) for b in begin]
        if len(begin) != 3:
            raise ValueError("block morphology: begin has three entries, not %s" % (begin,))
        return (C.c_int64 * 3)(*begin)

    def block_morphology_raw(self, labels, begin, cap):
        """One ctws_block_morphology call with an output of `cap` rows: (return code, n_rows,
        rows (cap, 11)).  labels is a 3-D uint64 array; the rows start out as NaN, so a call that
        writes nothing leaves them so."""
        labels = np.ascontiguousarray(labels, dtype=np.uint64)
        assert labels.ndim == 3 and labels.size, labels.shape
        rows = np.full((cap, 11), np.nan, dtype=np.float64)
        n = C.c_int64(0)
        ret = lib().ctws_block_morphology(self._h, labels.ctypes.data, *labels.shape, self._begin_arg(begin),
                                          rows.ctypes.data if cap else None, cap, C.byref(n))
        return ret, int(n.value), rows

    def block_morphology(self, labels, begin=(0, 0, 0)):
        """The morphology table of one block of uint64 labels at offset `begin` of its volume
        (include/ctws.h, ctws_block_morphology): rows (m, 11) float64 of [id, size, com_z, com_y,
        com_x, min_z, min_y, min_x, max_z, max_y, max_x], a row per id of the block (0 included),
        sorted by id, in global coordinates, minima and maxima inclusive.  A call that hits the
        capacity is repeated once with the returned size."""
        labels = np.asarray(labels)
        if labels.dtype != np.dtype('uint64'):
            raise TypeError("block morphology: the labels are uint64, not %s" % labels.dtype)
        if labels.ndim != 3 or not labels.size:
            raise ValueError("block morphology: the labels are a non-empty 3-D block, not %s" % (labels.shape,))
        m, rows = self._call_sized('ctws_block_morphology', (self.MORPHOLOGY_CAP,),
                                   lambda cap: self.block_morphology_raw(labels, begin, cap))
        return rows[:m]

    def block_morphology_device(self, labels, begin=(0, 0, 0)):
        """block_morphology on a uint64 / int64 torch tensor on this GPU; the rows come back as a
        float64 tensor on the same device: only their number crosses PCIe."""
        import torch
        assert labels.is_cuda and labels.is_contiguous() and labels.element_size() == 8 and labels.dim() == 3
        assert labels.numel() > 0 and not labels.is_floating_point()
        torch.cuda.current_stream(labels.device).synchronize()
        b = self._begin_arg(begin)
        n = C.c_int64(0)

        def call(cap):
            rows = torch.empty((cap, 11), dtype=torch.float64, device=labels.device)
            ret = lib().ctws_block_morphology_device(self._h, labels.data_ptr(), *labels.shape, b, rows.data_ptr(),
                                                     cap, C.byref(n))
            return ret, n.value, rows
        m, rows = self._call_sized('ctws_block_morphology_device', (self.MORPHOLOGY_CAP,), call)
        return rows[:m]

    # ---- RegionFeaturesWorkflow kernels ----------------------------------------------------
    # first capacity of region_features_block in rows: a call that does not fit computes everything again
    REGION_FEATURES_CAP = 1 << 16
    REGION_FEATURES_DTYPES = ('uint8', 'uint16', 'float32', 'float64')

    def region_features_block_raw(self, labels, data, ignore_label, cap):
        """One ctws_region_features_block call with an output of `cap` rows: (return code, n_rows,
        rows (cap, 3)).  labels is a 3-D uint64 array, data of the same shape (refused as
        region_features_block refuses them); the rows start out as NaN, so a call that writes
        nothing leaves them so."""
        labels = np.asarray(labels)
        data = np.asarray(data)
        self._region_features_check(labels.dtype, labels.shape, data.dtype, data.shape)
        labels = np.ascontiguousarray(labels)
        data = np.ascontiguousarray(data)
        rows = np.full((cap, 3), np.nan, dtype=np.float64)
        n = C.c_int64(0)
        wi, il = self._ignore_args(ignore_label)
        ret = lib().ctws_region_features_block(self._h, labels.ctypes.data, data.ctypes.data, dtype_code(data.dtype),
                                               *labels.shape, wi, il, rows.ctypes.data if cap else None, cap,
                                               C.byref(n))
        return ret, int(n.value), rows

    @classmethod
    def _region_features_check(cls, l_dtype, l_shape, d_dtype, d_shape):
        if _dtype_name(l_dtype) != 'uint64':
            raise TypeError("region features: the labels are uint64, not %s" % (l_dtype,))
        if _dtype_name(d_dtype) not in cls.REGION_FEATURES_DTYPES:
            raise TypeError("region features: the input map is uint8, uint16, float32 or float64, not %s"
                            % (d_dtype,))
        l_shape, d_shape = tuple(l_shape), tuple(d_shape)
        if l_shape != d_shape:
            raise ValueError("region features: labels and input map are of one shape, not %s and %s"
                             % (l_shape, d_shape))
        if len(l_shape) != 3 or 0 in l_shape:
            raise ValueError("region features: the labels are a non-empty 3-D block, not %s" % (l_shape,))

    def region_features_block(self, labels, data, ignore_label=0):
        """The region features of one block (include/ctws.h, ctws_region_features_block): labels
        (uint64) and data (uint8 taken as v / 255, uint16, float32 or float64, all as float32) of one
        3-D shape -> rows (m, 3) float64 of [id, count, mean], a row per id of the block, sorted by
        id.  ignore_label not None: that id's row, if it occurs, is [id, 0, 0].  A call that hits
        the capacity is repeated once with the returned size."""
        m, rows = self._call_sized('ctws_region_features_block', (self.REGION_FEATURES_CAP,),
                                   lambda cap: self.region_features_block_raw(labels, data, ignore_label, cap))
        return rows[:m]

    def region_features_block_device(self, labels, data, ignore_label=0):
        """region_features_block on torch tensors on this GPU: labels uint64 / int64 (the bits are
        taken as uint64), data uint8, uint16, float32 or float64; the rows come back as a float64
        tensor on the same device: only their number crosses PCIe."""
        import torch
        for t in (labels, data):
            assert t.is_cuda and t.is_contiguous()
        l_dtype = 'uint64' if labels.element_size() == 8 and not labels.is_floating_point() else labels.dtype
        self._region_features_check(l_dtype, labels.shape, data.dtype, data.shape)
        code = _dtype_code(data.dtype)
        torch.cuda.current_stream(labels.device).synchronize()
        wi, il = self._ignore_args(ignore_label)
        n = C.c_int64(0)

        def call(cap):
            rows = torch.empty((cap, 3), dtype=torch.float64, device=labels.device)
            ret = lib().ctws_region_features_block_device(self._h, labels.data_ptr(), data.data_ptr(), code,
                                                          *labels.shape, wi, il, rows.data_ptr(), cap, C.byref(n))
            return ret, n.value, rows
        m, rows = self._call_sized('ctws_region_features_block_device', (self.REGION_FEATURES_CAP,), call)
        return rows[:m]

    # ---- RegionCentersWorkflow kernels -------------------------------------------------------
    # boxes of at most this many voxels run one workgroup each with the transform in LDS
    # (ctws_kernels.h kRcSmallVox); timings() reports rc_small_objects / rc_large_objects
    REGION_CENTERS_SMALL_VOXELS = 10000

    @staticmethod
    def _resolution_arg(resolution):
        res = [float(r) for r in resolution]
        if len(res) != 3:
            raise ValueError("region centers: the resolution has three entries, not %s" % (resolution,))
        return (C.c_double * 3)(*res)

    def _region_centers_call(self, fn, labels_ptr, n_labels, ids, offsets, shapes, pitches, resolution, out):
        """One ctws_region_centers / _device call over object tables (ids (k,), offsets (k,), shapes
        (k, 3), pitches (k, 2)); out(k) -> (centers, found, their two pointers)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        k = len(ids)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        shapes = np.ascontiguousarray(shapes, dtype=np.int64).reshape(-1, 3)
        pitches = np.ascontiguousarray(pitches, dtype=np.int64).reshape(-1, 2)
        if not (len(offsets) == len(shapes) == len(pitches) == k):
            raise ValueError("region centers: %i ids, %i offsets, %i shapes, %i pitches"
                             % (k, len(offsets), len(shapes), len(pitches)))
        centers, found, pc, pf = out(k)
        ret = getattr(lib(), fn)(self._h, labels_ptr, int(n_labels), k, ids.ctypes.data, offsets.ctypes.data,
                                 shapes.ctypes.data, pitches.ctypes.data, self._resolution_arg(resolution), pc, pf)
        self._check(ret, fn)
        return centers, found

    @staticmethod
    def _region_centers_host_out(k):
        centers = np.zeros((k, 3), dtype=np.int64)
        found = np.zeros(k, dtype=np.uint8)
        return centers, found, centers.ctypes.data, found.ctypes.data

    @staticmethod
    def _box_tables(shape, boxes):
        """(k, 6) boxes [begin_z, begin_y, begin_x, end_z, end_y, end_x) inside a C-order volume of
        `shape` -> offsets, shapes, pitches of the call.  A box with end <= begin on an axis is
        empty; a box that leaves the volume is refused."""
        boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 6)
        Z, Y, X = (int(s) for s in shape)
        begin, end = boxes[:, :3], boxes[:, 3:]
        if len(boxes) and ((begin < 0).any() or (end > np.array([Z, Y, X])).any()):
            raise ValueError("region centers: a box leaves the volume of shape %s" % (tuple(shape),))
        shapes = np.maximum(end - begin, 0)
        offsets = (begin[:, 0] * Y + begin[:, 1]) * X + begin[:, 2]
        offsets = np.where((shapes == 0).any(axis=1), 0, offsets)
        pitches = np.tile(np.array([Y * X, X], dtype=np.int64), (len(boxes), 1))
        return offsets, shapes, pitches

    def region_centers(self, crops, ids, resolution=(1, 1, 1)):
        """The region centres of k objects given as crops (include/ctws.h, ctws_region_centers):
        crops is a list of 3-D uint64 arrays, one per object, packed into one buffer; ids (k,) the
        objects' ids.  -> (centers int64 (k, 3): per object the local (z, y, x) of the first voxel
        in C order with the largest exact squared distance to the crop's voxels of another label,
        scaled by the integer `resolution`; found bool (k,): False for an empty crop and for a crop
        without a voxel of its id, whose centre is (0, 0, 0))."""
        crops = [np.asarray(c) for c in crops]
        for c in crops:
            if c.dtype != np.dtype('uint64'):
                raise TypeError("region centers: the labels are uint64, not %s" % c.dtype)
            if c.ndim != 3:
                raise ValueError("region centers: a crop is 3-D, not %s" % (c.shape,))
        shapes = np.array([c.shape for c in crops], dtype=np.int64).reshape(-1, 3)
        sizes = shapes.prod(axis=1)
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if len(crops) else np.zeros(0, np.int64)
        pitches = np.stack([shapes[:, 1] * shapes[:, 2], shapes[:, 2]], axis=1)
        buf = np.empty(int(sizes.sum()), dtype=np.uint64)
        for c, o, n in zip(crops, offsets, sizes):
            buf[o:o + n] = c.reshape(-1)
        centers, found = self._region_centers_call('ctws_region_centers', buf.ctypes.data if buf.size else None,
                                                   buf.size, ids, offsets, shapes, pitches, resolution,
                                                   self._region_centers_host_out)
        return centers, found.astype(bool)

    def region_centers_boxes(self, labels, ids, boxes, resolution=(1, 1, 1)):
        """region_centers for (k, 6) boxes [begin, end) inside one 3-D uint64 array: the boxes are
        read in place at the array's pitches."""
        labels = np.asarray(labels)
        if labels.dtype != np.dtype('uint64'):
            raise TypeError("region centers: the labels are uint64, not %s" % labels.dtype)
        if labels.ndim != 3:
            raise ValueError("region centers: the labels are a 3-D array, not %s" % (labels.shape,))
        labels = np.ascontiguousarray(labels)
        offsets, shapes, pitches = self._box_tables(labels.shape, boxes)
        centers, found = self._region_centers_call('ctws_region_centers', labels.ctypes.data if labels.size else None,
                                                   labels.size, ids, offsets, shapes, pitches, resolution,
                                                   self._region_centers_host_out)
        return centers, found.astype(bool)

    def region_centers_boxes_device(self, labels, ids, boxes, resolution=(1, 1, 1)):
        """region_centers_boxes on a uint64 / int64 torch tensor on this GPU; centers (int64) and
        found (bool) come back as tensors on the same device."""
        import torch
        assert labels.is_cuda and labels.is_contiguous() and labels.element_size() == 8 and labels.dim() == 3
        assert not labels.is_floating_point()
        torch.cuda.current_stream(labels.device).synchronize()
        offsets, shapes, pitches = self._box_tables(labels.shape, boxes)

        def out(k):
            centers = torch.zeros((k, 3), dtype=torch.int64, device=labels.device)
            found = torch.zeros(k, dtype=torch.uint8, device=labels.device)
            return centers, found, centers.data_ptr(), found.data_ptr()
        centers, found = self._region_centers_call('ctws_region_centers_device',
                                                   labels.data_ptr() if labels.numel() else None, labels.numel(),
                                                   ids, offsets, shapes, pitches, resolution, out)
        return centers, found.bool()

    # ---- DownscalingWorkflow kernel ---------------------------------------------------------
    DOWNSCALE_DTYPES = ('uint8', 'uint16', 'float32', 'float64')
    DOWNSCALE_FUNCS = {'mean': 0, 'max': 1, 'min': 2}

    @classmethod
    def _downscale_check(cls, dtype, shape, factors, func):
        """The Python-side refusals of downscale_block: -> (factors, func code, output shape)."""
        if _dtype_name(dtype) not in cls.DOWNSCALE_DTYPES:
            raise TypeError("downscale: the block is uint8, uint16, float32 or float64, not %s" % (dtype,))
        shape = tuple(int(s) for s in shape)
        if len(shape) != 3 or 0 in shape:
            raise ValueError("downscale: the input is a non-empty 3-D block, not %s" % (shape,))
        try:
            fac = tuple(int(f) for f in factors)
            whole = all(f == g for f, g in zip(fac, factors))
        except TypeError:
            raise ValueError("downscale: factors are three integers in 1..8, not %r" % (factors,))
        if len(fac) != 3 or not whole or any(f < 1 or f > 8 for f in fac):
            raise ValueError("downscale: factors are three integers in 1..8, not %r" % (factors,))
        if func not in cls.DOWNSCALE_FUNCS:
            raise ValueError("downscale: func is 'mean', 'max' or 'min', not %r" % (func,))
        return fac, cls.DOWNSCALE_FUNCS[func], tuple(-(-s // f) for s, f in zip(shape, fac))

    def downscale_block_raw(self, x, factors, func, out):
        """One ctws_downscale_block call into `out` (a C-contiguous array of x's dtype): (return
        code, any_nonzero).  Nothing is refused here: the library's own checks answer."""
        x = np.ascontiguousarray(x)
        flag = C.c_int(-1)
        ret = lib().ctws_downscale_block(self._h, x.ctypes.data, dtype_code(x.dtype), *x.shape,
                                         (C.c_int64 * 3)(*[int(f) for f in factors]), int(func), out.ctypes.data,
                                         *out.shape, C.byref(flag))
        return ret, int(flag.value)

    def downscale_block(self, x, factors, func='mean'):
        """One block of a scale pyramid (include/ctws.h, ctws_downscale_block): x (nz, ny, nx) of
        uint8, uint16, float32 or float64, factors (fz, fy, fx) in 1..8, func 'mean', 'max' or 'min'
        -> (out, any_nonzero): out of shape ceil(n / f) per axis in x's dtype, as
        `skimage.measure.block_reduce` of the float32 block, clipped, rounded and cast; any_nonzero
        False when every voxel of x is zero."""
        x = np.asarray(x)
        fac, code, oshape = self._downscale_check(x.dtype, x.shape, factors, func)
        out = np.empty(oshape, dtype=x.dtype)
        ret, flag = self.downscale_block_raw(x, fac, code, out)
        self._check(ret, 'ctws_downscale_block')
        return out, bool(flag)

    def downscale_block_device(self, x, factors, func='mean'):
        """downscale_block on a torch tensor on this GPU; out comes back as a tensor of the same
        dtype on the same device: only the flag crosses PCIe."""
        import torch
        assert x.is_cuda and x.is_contiguous()
        fac, code, oshape = self._downscale_check(x.dtype, x.shape, factors, func)
        torch.cuda.current_stream(x.device).synchronize()
        out = torch.empty(oshape, dtype=x.dtype, device=x.device)
        flag = C.c_int(-1)
        ret = lib().ctws_downscale_block_device(self._h, x.data_ptr(), _dtype_code(x.dtype), *x.shape,
                                                (C.c_int64 * 3)(*fac), code, out.data_ptr(), *oshape, C.byref(flag))
        self._check(ret, 'ctws_downscale_block_device')
        return out, bool(flag.value)

    # ---- ImageFilter kernels ----------------------------------------------------------------
    IMAGE_FILTER_DTYPES = ('uint8', 'uint16', 'float32', 'float64')

    @classmethod
    def _image_filter_check(cls, dtype, shape, filter_name, sigma, apply_in_2d):
        fid, sig = image_filter_check(filter_name, sigma, apply_in_2d)
        if _dtype_name(dtype) not in cls.IMAGE_FILTER_DTYPES:
            raise TypeError("image filter: the block is uint8, uint16, float32 or float64, not %s" % (dtype,))
        shape = tuple(int(s) for s in shape)
        if len(shape) != 3 or 0 in shape:
            raise ValueError("image filter: the input is a non-empty 3-D block, not %s" % (shape,))
        return fid, (C.c_double * 3)(*sig), shape

    def image_filter(self, data, filter_name, sigma, apply_in_2d=False, normalize=True):
        """One block through a Gaussian filter (include/ctws.h, ctws_image_filter): data (nz, ny, nx)
        of uint8, uint16, float32 or float64; filter_name 'gaussianSmoothing',
        'gaussianGradientMagnitude' or 'laplacianOfGaussian'; sigma a positive scalar or (z, y, x);
        apply_in_2d filters every z slice on its own; normalize applies vu.normalize to the block
        first.  -> the float32 response of the same shape.  A block shorter than a tap radius + 1
        along a filtered axis raises CtwsError."""
        data = np.ascontiguousarray(data)
        fid, sig, shape = self._image_filter_check(data.dtype, data.shape, filter_name, sigma, apply_in_2d)
        out = np.empty(shape, dtype=np.float32)
        ret = lib().ctws_image_filter(self._h, data.ctypes.data, dtype_code(data.dtype), *shape, fid, sig,
                                      int(bool(apply_in_2d)), int(bool(normalize)), out.ctypes.data)
        self._check(ret, 'ctws_image_filter')
        return out

    def image_filter_device(self, data, filter_name, sigma, apply_in_2d=False, normalize=True):
        """image_filter on a torch tensor on this GPU; the response comes back as a float32 tensor
        on the same device: nothing crosses PCIe."""
        import torch
        assert data.is_cuda and data.is_contiguous()
        fid, sig, shape = self._image_filter_check(data.dtype, data.shape, filter_name, sigma, apply_in_2d)
        torch.cuda.current_stream(data.device).synchronize()
        out = torch.empty(shape, dtype=torch.float32, device=data.device)
        ret = lib().ctws_image_filter_device(self._h, data.data_ptr(), _dtype_code(data.dtype), *shape, fid, sig,
                                             int(bool(apply_in_2d)), int(bool(normalize)), out.data_ptr())
        self._check(ret, 'ctws_image_filter_device')
        return out

    # ---- multi-GPU label-count exchange (RCCL) ------------------------------------------
