"""rsx — Python host binding of librsx.so (include/rsx.h), the MI355X dense-retrieval engine.

The module exposes the subset of the `faiss` Python surface that the reference's search path
uses (every call site listed in SURVEY.md §2.2), with the same names, argument meaning and error
behaviour, so `src/indicies/*.py` is written against `rsx` exactly as the reference's files are
written against `faiss`:

    reference                                          here
    faiss.IndexFlatIP(d)            flat.py:42         rsx.IndexFlatIP(d)
    faiss.IndexIVFFlat(q,d,nlist,METRIC_INNER_PRODUCT) ivf_flat.py:144   rsx.IndexIVFFlat(...)
    faiss.IndexIVFPQ(q,d,nlist,M,nbits,METRIC_IP)      ivf_pq.py:147     rsx.IndexIVFPQ(...)
    faiss.IndexPQ(d,M,nbits,METRIC_IP)    contriever/src/index.py:19     rsx.IndexPQ(...)
    faiss.IndexScalarQuantizer(d,QT_8bit,metric)  (factory "SQ8")          rsx.IndexScalarQuantizer(...)
    faiss.IndexRefineFlat(base)           (factory "...,RFlat")          rsx.IndexRefineFlat(base)
    index.reconstruct / reconstruct_batch / reconstruct_n / search_and_reconstruct / make_direct_map
        (faiss.Index verbs; the reference's get_embs(indices))            same, decoded on the GPU
    index.train / add / search / nprobe / ntotal / is_trained            same
    index.range_search(x, radius)         (faiss.Index verb; Flat, IVF-Flat) same, lims as int64
    faiss.read_index / write_index                                        rsx.read_index / write_index
    faiss.VectorTransform / LinearTransform / RandomRotationMatrix / PCAMatrix / OPQMatrix, IndexPreTransform,
        index_factory, extract_index_ivf, downcast_index  (factory "OPQ96,IVF4096,PQ96")   same names (module rsx_vt, re-exported here)
    StandardGpuResources / GpuClonerOptions / index_cpu_to_gpu / index_gpu_to_cpu
        (ivf_flat.py:155-163: CUDA-only training clone)                   identity shims — the index
                                                                          already lives on the GPU

All arithmetic happens in the HIP library.  There is NO CPU fallback: importing works without a
GPU (so host logic can be tested), but constructing an index raises RuntimeError unless librsx.so
is built and a HIP device is present.
"""
import ctypes
import os
import subprocess

import numpy as np

METRIC_INNER_PRODUCT = 0
METRIC_L2 = 1

_F32, _F16 = 0, 1
_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_LIB_PATH = os.environ.get("RSX_LIB", os.path.join(_CSRC, "librsx.so"))   # RSX_LIB: another build, for A/B measurements
_lib = None

#: every symbol include/rsx.h declares (checked by tests/test_abi.py against the header)
ABI_SYMBOLS = [
    "rsx_last_error", "rsx_version", "rsx_device_count", "rsx_flat_create", "rsx_ivfflat_create",
    "rsx_ivfpq_create", "rsx_pq_create", "rsx_sharded_create", "rsx_load_sharded", "rsx_destroy", "rsx_train", "rsx_set_centroids", "rsx_set_codebooks",
    "rsx_get_centroids", "rsx_get_codebooks", "rsx_add", "rsx_assign", "rsx_reset", "rsx_reserve_lists", "rsx_add_list",
    "rsx_get_list", "rsx_get_list_sizes", "rsx_set_nprobe", "rsx_search", "rsx_search_prepass", "rsx_search_scan", "rsx_merge_topk", "rsx_pack_topk", "rsx_merge_packed", "rsx_get",
    "rsx_set_param",
    "rsx_get_timing", "rsx_save", "rsx_load", "rsx_synth_vectors", "rsx_synth_queries",
    "rsx_selector_create", "rsx_selector_destroy", "rsx_selector_is_member", "rsx_search_sel", "rsx_search_prepass_sel",
    "rsx_remove_ids", "rsx_refine",
    "rsx_ivfsq_create", "rsx_set_sq_trained", "rsx_get_sq_trained", "rsx_sq_create",
    "rsx_range_search", "rsx_range_result_get", "rsx_range_result_destroy",
    "rsx_make_direct_map", "rsx_reconstruct_batch",
    "rsx_vt_create", "rsx_vt_set", "rsx_vt_apply", "rsx_vt_destroy",
    "rsx_merge_from", "rsx_copy_subset_to",
]


def build(force=False, verbose=False):
    """Compile librsx.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", _CSRC, "-j8"]
    if force:
        args.append("-B")
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(args, stdout=out)
    return _LIB_PATH


def lib():
    """The loaded C-ABI library; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the search path)")
        # PyTorch-ROCm ships its own libamdhip64: whichever copy is mapped FIRST serves the whole process (same soname), and a
        # process that maps /opt/rocm's through librsx and torch's afterwards ends up with two HIP runtimes — torch then
        # reports "No HIP GPUs are available".  Load torch's first whenever torch is installed.
        if not os.environ.get("RSX_NO_TORCH"):
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = ctypes.CDLL(_LIB_PATH)
        L.rsx_last_error.restype = ctypes.c_char_p
        for name in ABI_SYMBOLS:
            getattr(L, name)  # AttributeError if the library does not export it
        _lib = L
    return _lib


def _check(status):
    if status != 0:
        msg = lib().rsx_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"rsx error {status}: {msg}")


def get_num_gpus():
    n = ctypes.c_int(0)
    st = lib().rsx_device_count(ctypes.byref(n))
    return n.value if st == 0 else 0


def default_device():
    for key in ("RSX_DEVICE", "LOCAL_RANK"):
        if key in os.environ:
            return int(os.environ[key])
    return 0


_default_devices = None


def set_default_devices(devices):
    """Devices new indexes span when no `device` / `devices` argument is given: a list of ordinals (one shard per
    entry, single process — rsx_sharded_create), "all", or None for one GPU.  The Indexer facade sets this from
    cfg.datastore.index.devices; the RSX_DEVICES environment variable ("0,1,2,3" or "all") is the fallback."""
    global _default_devices
    _default_devices = devices


def get_default_devices():
    return _default_devices


def _resolve_devices(device, devices):
    """-> None (single-GPU handle on `device`) or a list of device ordinals (sharded handle)."""
    if devices is None and device is None:
        devices = _default_devices
        if devices is None and os.environ.get("RSX_DEVICES"):
            devices = os.environ["RSX_DEVICES"]
    if devices is None:
        return None
    if isinstance(devices, str):
        devices = list(range(get_num_gpus())) if devices.strip().lower() == "all" else [int(t) for t in devices.split(",") if t.strip()]
    devices = [int(t) for t in devices]
    return devices or None


def _create(kind, d, nlist, M, nbits, metric, device, devices):
    h = ctypes.c_void_p()
    devs = _resolve_devices(device, devices)
    if devs is not None and len(devs) > 1:
        arr = (ctypes.c_int * len(devs))(*devs)
        _check(lib().rsx_sharded_create(kind, int(d), int(nlist), int(M), int(nbits), int(metric), len(devs), arr, ctypes.byref(h)))
        return h
    if devs is not None:           # a one-entry list ("2", [2]) names the device of an ordinary handle
        device = devs[0]
    dev = default_device() if device is None else int(device)
    if kind == 0:
        _check(lib().rsx_flat_create(int(d), int(metric), dev, ctypes.byref(h)))
    elif kind == 1:
        _check(lib().rsx_ivfflat_create(int(d), int(nlist), int(metric), dev, ctypes.byref(h)))
    elif kind == 3:
        _check(lib().rsx_pq_create(int(d), int(M), int(nbits), int(metric), dev, ctypes.byref(h)))
    else:
        _check(lib().rsx_ivfpq_create(int(d), int(nlist), int(M), int(nbits), int(metric), dev, ctypes.byref(h)))
    return h


# ------------------------------------------------------------------------------------------
# array plumbing: numpy (host) or torch CUDA tensors (HBM) -> raw pointers
# ------------------------------------------------------------------------------------------
def _is_torch(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _as_matrix(x, d, what):
    """-> (keepalive, pointer, n, dtype_code, on_device).  Mirrors faiss's SWIG wrapper: 2-D,
    C-contiguous, second dimension d; fp32 (FAISS) or fp16 (kept as is — no up-cast needed)."""
    if _is_torch(x):
        import torch
        if x.dim() != 2 or x.shape[1] != d:
            raise AssertionError(f"{what}: expected shape [n, {d}], got {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.float16):
            x = x.float()
        x = x.contiguous()
        return x, ctypes.c_void_p(x.data_ptr()), x.shape[0], (_F16 if x.dtype == torch.float16 else _F32), x.is_cuda
    x = np.asarray(x)
    if x.ndim != 2 or x.shape[1] != d:
        raise AssertionError(f"{what}: expected shape [n, {d}], got {x.shape}")
    if x.dtype not in (np.float32, np.float16):
        x = x.astype(np.float32)
    x = np.ascontiguousarray(x)
    return x, ctypes.c_void_p(x.ctypes.data), x.shape[0], (_F16 if x.dtype == np.float16 else _F32), False


def _sync_producer(keep, on_dev):
    """The library reads caller data on its OWN (non-blocking) stream: a CUDA tensor must be complete before the
    call — including the .float()/.contiguous() copies _as_matrix may have enqueued on torch's current stream."""
    if on_dev:
        import torch
        torch.cuda.current_stream(keep.device).synchronize()


# ------------------------------------------------------------------------------------------
# filtered search: faiss.IDSelector* and faiss.SearchParameters* (FAISS 1.8.0 names)
# ------------------------------------------------------------------------------------------
_SEL_RANGE, _SEL_BATCH, _SEL_BITMAP = 0, 1, 2


class IDSelector:
    """Base of the id selectors.  A selector is immutable; its native object (rsx_selector_create, host memory only) is built
    on first use and cached, so a selector reused across searches keeps the slot mask an index caches for it."""

    _native_h = None

    def _spec(self):
        """-> (kind, data array or None, lo, hi, invert)"""
        raise NotImplementedError

    def _native(self):
        if self._native_h is None:
            kind, data, lo, hi, inv = self._spec()
            h = ctypes.c_void_p()
            ptr = data.ctypes.data_as(ctypes.c_void_p) if data is not None and data.size else None
            n = 0 if data is None else data.size
            _check(lib().rsx_selector_create(kind, ptr, ctypes.c_int64(n), ctypes.c_int64(lo), ctypes.c_int64(hi), int(inv), ctypes.byref(h)))
            self._native_h = h
        return self._native_h

    def __del__(self):
        h = self._native_h
        if h is not None and _lib is not None:
            try:
                _lib.rsx_selector_destroy(h)
            except Exception:
                pass
            self._native_h = None

    def is_member(self, ids):
        """bool array: which of the int64 `ids` the selector selects (host code, no GPU)."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int64)
        out = np.zeros(ids.shape, dtype=np.uint8)
        _check(lib().rsx_selector_is_member(self._native(), ctypes.c_int64(ids.size), ids.ctypes.data_as(ctypes.c_void_p),
                                            out.ctypes.data_as(ctypes.c_void_p)))
        return out.astype(bool)

    def shifted(self, offset, n_local=None):
        """The selector over LOCAL ids i of a shard whose ids are the global ids i + offset (n_local: the shard's id count, lets a
        bitmap or batch keep only the shard's part).  Used by sharded.ShardedSearcher for id-range shards."""
        raise NotImplementedError


class IDSelectorRange(IDSelector):
    """faiss.IDSelectorRange(imin, imax): ids in [imin, imax)."""

    def __init__(self, imin, imax):
        self.imin, self.imax = int(imin), int(imax)

    def _spec(self):
        return _SEL_RANGE, None, self.imin, self.imax, False

    def shifted(self, offset, n_local=None):
        return IDSelectorRange(self.imin - offset, self.imax - offset) if offset else self


class IDSelectorBatch(IDSelector):
    """faiss.IDSelectorBatch(ids) or (n, ids): any int64 ids; duplicates allowed, ids absent from the index ignored."""

    def __init__(self, *args):
        ids = args[-1]
        if _is_torch(ids):
            ids = ids.detach().cpu().numpy()
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if len(args) == 2:
            ids = ids[: int(args[0])]
        elif len(args) != 1:
            raise TypeError("IDSelectorBatch(ids) or IDSelectorBatch(n, ids)")
        self.ids = ids

    def _spec(self):
        return _SEL_BATCH, self.ids, 0, 0, False

    def shifted(self, offset, n_local=None):
        if not offset and n_local is None:
            return self
        loc = self.ids - offset
        if n_local is not None:
            loc = loc[(loc >= 0) & (loc < n_local)]
        return IDSelectorBatch(loc)


class IDSelectorBitmap(IDSelector):
    """faiss.IDSelectorBitmap(bitmap) or (n, bitmap): uint8 [n]; id i is selected when i < 8 n and bit i & 7 (least significant
    first) of byte i >> 3 is set."""

    def __init__(self, *args):
        bm = args[-1]
        if _is_torch(bm):
            bm = bm.detach().cpu().numpy()
        bm = np.ascontiguousarray(bm).reshape(-1)
        if bm.dtype != np.uint8:
            raise TypeError(f"IDSelectorBitmap: bitmap must be uint8, got {bm.dtype}")
        if len(args) == 2:
            bm = bm[: int(args[0])]
        elif len(args) != 1:
            raise TypeError("IDSelectorBitmap(bitmap) or IDSelectorBitmap(n, bitmap)")
        self.bitmap = bm

    def _spec(self):
        return _SEL_BITMAP, self.bitmap, 0, 0, False

    def shifted(self, offset, n_local=None):
        if not offset and n_local is None:
            return self
        nbits = 8 * self.bitmap.size
        end = nbits if n_local is None else min(nbits, offset + int(n_local))
        if offset % 8 == 0:
            return IDSelectorBitmap(self.bitmap[offset // 8:(end + 7) // 8] if end > offset else np.zeros(0, np.uint8))
        if end <= max(offset, 0):
            return IDSelectorBitmap(np.zeros(0, np.uint8))
        lo = max(offset, 0)       # only the shard's own bits are unpacked (local ids below -offset cannot exist)
        bits = np.unpackbits(self.bitmap[lo // 8:(end + 7) // 8], bitorder="little")[lo % 8:lo % 8 + (end - lo)]
        if lo > offset:
            bits = np.concatenate([np.zeros(lo - offset, np.uint8), bits])
        return IDSelectorBitmap(np.packbits(bits, bitorder="little"))


class IDSelectorNot(IDSelector):
    """faiss.IDSelectorNot(sel): the complement of another selector."""

    def __init__(self, sel):
        if not isinstance(sel, IDSelector):
            raise TypeError(f"IDSelectorNot takes an IDSelector, got {type(sel).__name__}")
        self.sel = sel

    def _spec(self):
        kind, data, lo, hi, inv = self.sel._spec()
        return kind, data, lo, hi, not inv

    def shifted(self, offset, n_local=None):
        # the complement must stay a complement over ALL local ids: no truncation to the shard's part
        return IDSelectorNot(self.sel.shifted(offset, None)) if offset else self


def _remove_selector(x):
    """Index.remove_ids argument -> IDSelector: a selector as is, a 1-D integer array as IDSelectorBatch(x)."""
    if isinstance(x, IDSelector):
        return x
    if _is_torch(x):
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.ndim != 1:
        raise ValueError(f"remove_ids: expected an IDSelector or a 1-D array of ids, got an array of shape {a.shape}")
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"remove_ids: ids must be integers, got {a.dtype}")
    return IDSelectorBatch(a.astype(np.int64))


class SearchParameters:
    """faiss.SearchParameters(sel=None): per-call parameters of Index.search (Flat)."""

    def __init__(self, sel=None):
        self.sel = sel


class SearchParametersIVF(SearchParameters):
    """faiss.SearchParametersIVF(sel=None, nprobe=1, max_codes=0): IVF-Flat / IVF-PQ.  As in FAISS 1.8.0 nprobe defaults to 1 and
    replaces index.nprobe for the call only.  max_codes and quantizer_params are not implemented: a non-default value is refused."""

    def __init__(self, sel=None, nprobe=1, max_codes=0, quantizer_params=None):
        super().__init__(sel)
        self.nprobe = nprobe
        self.max_codes = max_codes
        self.quantizer_params = quantizer_params


def _resolve_params(params, is_ivf):
    """-> (native selector or None, nprobe override (0 = none), keepalive).  FAISS 1.8.0's type rules: IndexIVF::search
    refuses a params object that is not SearchParametersIVF ("IndexIVF params have incorrect type")."""
    if not isinstance(params, SearchParameters):
        raise TypeError(f"params must be a SearchParameters object, got {type(params).__name__}")
    if is_ivf and not isinstance(params, SearchParametersIVF):
        raise RuntimeError("IndexIVF params have incorrect type")
    nprobe = 0
    if isinstance(params, SearchParametersIVF):
        if params.max_codes:
            raise NotImplementedError(f"SearchParametersIVF.max_codes = {params.max_codes}: not implemented (only the default 0)")
        if params.quantizer_params is not None:
            raise NotImplementedError("SearchParametersIVF.quantizer_params: not implemented")
        if is_ivf:
            nprobe = int(params.nprobe)
            if nprobe <= 0:
                raise ValueError(f"SearchParametersIVF.nprobe must be positive, got {params.nprobe}")
    sel = params.sel
    if sel is None:
        return None, nprobe, None
    if not isinstance(sel, IDSelector):
        raise TypeError(f"params.sel must be an IDSelector, got {type(sel).__name__}")
    return sel._native(), nprobe, sel


class Index:
    """Base handle.  Attributes follow faiss.Index: d, ntotal, is_trained, metric_type."""

    @property
    def nshards(self):
        """0 for a single-GPU handle, else the number of per-device shards behind this (single-process) handle."""
        return self._get("nshards")

    def __init__(self, handle, d, metric):
        self._h = handle
        self.d = d
        self.metric_type = metric

    # -- lifetime
    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib is not None:
            try:
                _lib.rsx_destroy(h)
            except Exception:
                pass
            self._h = None

    # -- properties
    def _get(self, key):
        v = ctypes.c_int64(0)
        _check(lib().rsx_get(self._h, key.encode(), ctypes.byref(v)))
        return v.value

    @property
    def ntotal(self):
        return self._get("ntotal")

    @property
    def is_trained(self):
        return bool(self._get("is_trained"))

    @property
    def storage_dtype(self):
        if self._get("kind") in (4, 5):
            return "sq8"
        return {0: "float32", 1: "float16", -1: "pq"}[self._get("storage_dtype")]

    def set_param(self, key, value):
        _check(lib().rsx_set_param(self._h, key.encode(), ctypes.c_double(value)))

    def get_timing(self, key):
        v = ctypes.c_double(0)
        _check(lib().rsx_get_timing(self._h, key.encode(), ctypes.byref(v)))
        return v.value

    # -- faiss.Index API
    def train(self, x):
        keep, p, n, dt, on_dev = _as_matrix(x, self.d, "train")
        _sync_producer(keep, on_dev)
        _check(lib().rsx_train(self._h, ctypes.c_int64(n), p, dt))

    def add(self, x):
        keep, p, n, dt, on_dev = _as_matrix(x, self.d, "add")
        _sync_producer(keep, on_dev)
        _check(lib().rsx_add(self._h, ctypes.c_int64(n), p, dt, None))

    def reset(self):
        _check(lib().rsx_reset(self._h))

    def add_with_ids(self, x, ids):
        keep, p, n, dt, on_dev = _as_matrix(x, self.d, "add_with_ids")
        _sync_producer(keep, on_dev)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        assert ids.shape == (n,), "ids must have one entry per vector"
        _check(lib().rsx_add(self._h, ctypes.c_int64(n), p, dt, ids.ctypes.data_as(ctypes.c_void_p)))

    def remove_ids(self, x):
        """faiss.Index.remove_ids(x) -> int, the number of vectors removed.  x: an IDSelector, or a 1-D integer array of ids (made
        an IDSelectorBatch, as FAISS's replacement_remove_ids does; duplicates and absent ids are allowed).  IVF lists fill each
        hole with their last entry (FAISS's in-list order); Flat compacts in order, renumbering sequential ids (rsx_remove_ids)."""
        sel = _remove_selector(x)
        n = ctypes.c_int64(0)
        _check(lib().rsx_remove_ids(self._h, sel._native(), ctypes.byref(n)))
        return int(n.value)

    def merge_from(self, other, add_id=0):
        """faiss.Index.merge_from(other, add_id): every entry of `other` moves behind this index's own (per list, in other's order, ids
        stored as id + add_id) and `other` ends empty.  On the GPU, without a pass through the host (rsx_merge_from).  Both must be
        unsharded handles of one kind on one device with bit-equal trained parameters; Flat-codes kinds (IndexFlat* of sequential ids,
        IndexPQ, IndexScalarQuantizer) take add_id = 0 only."""
        if not isinstance(other, Index):
            raise TypeError(f"merge_from: the other index must be an rsx index handle, got {type(other).__name__}")
        _check(lib().rsx_merge_from(self._h, other._h, ctypes.c_int64(int(add_id))))

    def search(self, x, k, *, params=None):
        """-> (D float32 [n,k], I int64 [n,k]); numpy in -> numpy out, CUDA tensor in -> CUDA tensors out.
        params: SearchParameters (Flat) / SearchParametersIVF (IVF) — a filtered search returns what the unfiltered search of an
        index holding only the selected vectors returns (rsx_search_sel)."""
        keep, p, n, dt, on_dev = _as_matrix(x, self.d, "search")
        k = int(k)
        assert k > 0, "k must be positive"
        if params is not None:
            sel, nprobe, sel_keep = _resolve_params(params, isinstance(self, _IndexIVF))

            def call(Dp, Ip):
                _check(lib().rsx_search_sel(self._h, ctypes.c_int64(n), p, dt, k, sel, int(nprobe), Dp, Ip))
        else:
            def call(Dp, Ip):
                _check(lib().rsx_search(self._h, ctypes.c_int64(n), p, dt, k, Dp, Ip))
        if on_dev:
            import torch
            D = torch.empty((n, k), dtype=torch.float32, device=keep.device)
            I = torch.empty((n, k), dtype=torch.int64, device=keep.device)
            _sync_producer(keep, on_dev)
            call(ctypes.c_void_p(D.data_ptr()), ctypes.c_void_p(I.data_ptr()))
            return D, I
        D = np.empty((n, k), dtype=np.float32)
        I = np.empty((n, k), dtype=np.int64)
        call(D.ctypes.data_as(ctypes.c_void_p), I.ctypes.data_as(ctypes.c_void_p))
        return D, I

    def range_search(self, x, radius, *, params=None):
        """faiss.Index.range_search(x, radius) -> (lims, D, I): every stored vector with score > radius (inner product) or squared
        distance < radius (L2) — strict, on the exact fp32 value `search` returns for that row; IVF-Flat over the rows of the nprobe
        probed lists.  lims int64 [n + 1] with lims[0] = 0: query i owns D[lims[i]:lims[i+1]] (float32) and I[lims[i]:lims[i+1]] (int64),
        best first, equal values by id ascending.  FAISS returns lims as uint64; int64 here, so that CUDA tensors can carry it.
        numpy in -> numpy out, CUDA tensor in -> CUDA tensors out.  IndexFlat* and IndexIVFFlat only (rsx_range_search); params:
        SearchParameters / SearchParametersIVF without a selector (nprobe replaces index.nprobe for the call)."""
        if not isinstance(self, (IndexFlat, IndexIVFFlat)):
            raise RuntimeError(f"range_search: not available on {type(self).__name__} in this build (IndexFlat* and IndexIVFFlat only)")
        nprobe = 0
        if params is not None:
            sel, nprobe, _ = _resolve_params(params, isinstance(self, _IndexIVF))
            if sel is not None:
                raise RuntimeError("range_search: a params object that carries a selector is not supported in this build")
        keep, p, n, dt, on_dev = _as_matrix(x, self.d, "range_search")
        _sync_producer(keep, on_dev)
        r = ctypes.c_void_p()
        _check(lib().rsx_range_search(self._h, ctypes.c_int64(n), p, dt, ctypes.c_float(float(radius)), int(nprobe), ctypes.byref(r)))
        try:
            total, dev = ctypes.c_int64(0), ctypes.c_int(0)
            pl, pD, pI = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            _check(lib().rsx_range_result_get(r, None, ctypes.byref(total), ctypes.byref(dev), ctypes.byref(pl), ctypes.byref(pD), ctypes.byref(pI)))
            total = total.value
            if dev.value:      # the result lives in device memory: cloned into tensors before it is destroyed
                import torch

                def take(ptr, count, typestr, dtype):
                    if count == 0 or not ptr.value:
                        return torch.empty((0,), dtype=dtype, device=keep.device)

                    class _View:      # the library's memory through the CUDA array interface
                        __cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr.value, False), "version": 2}
                    return torch.as_tensor(_View(), device=keep.device).clone()
                out = take(pl, n + 1, "<i8", torch.int64), take(pD, total, "<f4", torch.float32), take(pI, total, "<i8", torch.int64)
                torch.cuda.current_stream(keep.device).synchronize()
                return out if on_dev else tuple(a.cpu().numpy() for a in out)

            def take(ptr, count, ctype, dtype):
                if count == 0 or not ptr.value:
                    return np.empty((0,), dtype=dtype)
                return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(count,)).astype(dtype, copy=True)
            out = take(pl, n + 1, ctypes.c_int64, np.int64), take(pD, total, ctypes.c_float, np.float32), take(pI, total, ctypes.c_int64, np.int64)
            if on_dev:         # a host result for CUDA-tensor queries (an empty batch has no device pointer to tell by): tensors on the queries' device
                import torch
                return tuple(torch.as_tensor(a).to(keep.device) for a in out)
            return out
        finally:
            lib().rsx_range_result_destroy(r)

    def search_prepass(self, x, k, params=None):
        """First half of a two-call search (rsx_search_prepass): CUDA-tensor queries in -> a CUDA int64 tensor VIEW of the nq
        threshold keys (or None when this search has none).  The keys are unsigned 64-bit integers: flip the sign bit
        (`t ^= -2**63`) before comparing / reducing them as int64 and flip it back afterwards.  Finish with search_scan()."""
        import torch
        keep, p, n, dt, on_dev = _as_matrix(x, self.d, "search")
        assert on_dev, "search_prepass takes CUDA-tensor queries (the thresholds live in HBM)"
        k = int(k)
        D = torch.empty((n, k), dtype=torch.float32, device=keep.device)
        I = torch.empty((n, k), dtype=torch.int64, device=keep.device)
        _sync_producer(keep, on_dev)
        tau, ntau = ctypes.c_void_p(), ctypes.c_int64(0)
        if params is not None:      # (a filtered search has no threshold pre-pass: None comes back)
            sel, nprobe, sel_keep = _resolve_params(params, isinstance(self, _IndexIVF))
            _check(lib().rsx_search_prepass_sel(self._h, ctypes.c_int64(n), p, dt, k, sel, int(nprobe), ctypes.c_void_p(D.data_ptr()),
                                                ctypes.c_void_p(I.data_ptr()), ctypes.byref(tau), ctypes.byref(ntau)))
            self._two_call_sel = sel_keep      # the selector outlives the worker that reads it
        else:
            _check(lib().rsx_search_prepass(self._h, ctypes.c_int64(n), p, dt, k, ctypes.c_void_p(D.data_ptr()), ctypes.c_void_p(I.data_ptr()),
                                            ctypes.byref(tau), ctypes.byref(ntau)))
        self._two_call = (keep, D, I)
        if not tau.value or ntau.value == 0:
            return None

        class _View:      # zero-copy view of library memory through the CUDA array interface
            __cuda_array_interface__ = {"shape": (ntau.value,), "typestr": "<i8", "data": (tau.value, False), "version": 2}
        return torch.as_tensor(_View(), device=keep.device)

    def search_scan(self):
        """Second half: runs the scan with the (possibly raised) thresholds -> (D, I) CUDA tensors."""
        keep, D, I = self._two_call
        self._two_call = None
        try:
            _check(lib().rsx_search_scan(self._h))
        finally:
            self._two_call_sel = None
        return D, I

    # -- inspection (parity tests, writer)
    def get_list(self, list_no=0):
        """-> (payload, ids): IVFPQ payload = codes uint8 [n, M]; IVFSQ / IndexScalarQuantizer payload = codes uint8 [n, d]; Flat/IVFFlat payload = float32 [n, d]."""
        n = ctypes.c_int64(0)
        _check(lib().rsx_get_list(self._h, ctypes.c_int64(list_no), ctypes.byref(n), None, None))
        n = n.value
        if self._get("kind") in (2, 3):
            payload = np.empty((n, self._get("M")), dtype=np.uint8)
        elif self._get("kind") in (4, 5):
            payload = np.empty((n, self.d), dtype=np.uint8)
        else:
            payload = np.empty((n, self.d), dtype=np.float32)
        ids = np.empty(n, dtype=np.int64)
        if n:
            _check(lib().rsx_get_list(self._h, ctypes.c_int64(list_no), None, payload.ctypes.data_as(ctypes.c_void_p),
                                      ids.ctypes.data_as(ctypes.c_void_p)))
        return payload, ids

    def list_sizes(self):
        """int64 [nlist]: vectors per inverted list (Flat: one entry = ntotal) — the bench's list-length histogram."""
        out = np.zeros(max(1, self._get("nlist")), dtype=np.int64)
        _check(lib().rsx_get_list_sizes(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    # -- stored vectors by id (rsx_reconstruct_batch)
    def _reconstruct_keys(self, keys, fill_negative):
        """keys: int64, numpy (-> numpy float32 [n, d]) or a CUDA tensor (-> CUDA tensor); any shape, read flattened."""
        if _is_torch(keys) and keys.is_cuda:
            import torch
            k = keys.to(torch.int64).contiguous().reshape(-1)
            out = torch.empty((k.numel(), self.d), dtype=torch.float32, device=k.device)
            _sync_producer(k, True)
            _check(lib().rsx_reconstruct_batch(self._h, ctypes.c_int64(k.numel()), ctypes.c_void_p(k.data_ptr()) if k.numel() else None,
                                               int(fill_negative), ctypes.c_void_p(out.data_ptr()) if k.numel() else None))
            return out
        back = _is_torch(keys)
        k = np.ascontiguousarray(keys.numpy() if back else keys, dtype=np.int64).reshape(-1)
        out = np.empty((len(k), self.d), dtype=np.float32)
        _check(lib().rsx_reconstruct_batch(self._h, ctypes.c_int64(len(k)), k.ctypes.data_as(ctypes.c_void_p) if len(k) else None,
                                           int(fill_negative), out.ctypes.data_as(ctypes.c_void_p) if len(k) else None))
        if back:
            import torch
            return torch.from_numpy(out)
        return out

    def reconstruct_batch(self, keys):
        """faiss.Index.reconstruct_batch(keys) -> float32 [n, d]: the vector the index STORES for every key (an id, the label `search`
        returns), in the order of the keys; keys may repeat.  Flat / IVF-Flat: the stored row; IVF-PQ: centroid + codebook entries
        (the decoded vector, not the one that was added); IndexPQ: the codebook entries; IVF-SQ: the decoded code (+ centroid with
        by_residual).  numpy keys -> numpy out, a CUDA int64 tensor -> a CUDA tensor.  A key that is not stored raises (the message
        names the first one).  Unlike FAISS's IndexIVF no make_direct_map() is needed first: the first lookup builds the map."""
        return self._reconstruct_keys(keys, False)

    def reconstruct(self, key):
        """faiss.Index.reconstruct(key) -> float32 [d]."""
        return self._reconstruct_keys(np.array([int(key)], dtype=np.int64), False)[0]

    def reconstruct_n(self, i0=0, n=None):
        """faiss.Index.reconstruct_n(i0, n) = reconstruct_batch(arange(i0, i0 + n)); n None: up to ntotal."""
        n = self.ntotal - int(i0) if n is None else int(n)
        assert n >= 0, "reconstruct_n: n must not be negative"
        return self._reconstruct_keys(np.arange(int(i0), int(i0) + n, dtype=np.int64), False)

    def search_and_reconstruct(self, x, k, *, params=None):
        """faiss.Index.search_and_reconstruct(x, k) -> (D, I, R float32 [n, k, d]): D, I exactly what search(x, k, params=params)
        returns, R[i, j] = reconstruct(I[i, j]); where I[i, j] = -1 every bit of R[i, j] is set (FAISS's memset(-1); reads as NaN).
        The labels stay on the device between the search and the gather.  numpy in -> numpy out, CUDA tensor in -> CUDA tensors out."""
        import torch
        on_dev = _is_torch(x) and x.is_cuda
        if on_dev:
            xq = x
        else:
            xh = x if _is_torch(x) else np.asarray(x)
            if not _is_torch(xh) and xh.dtype not in (np.float32, np.float16):
                xh = xh.astype(np.float32)
            xq = torch.as_tensor(xh).to(f"cuda:{self._get('device')}")
        D, I = self.search(xq, k, params=params)
        R = self._reconstruct_keys(I, True).reshape(I.shape[0], I.shape[1], self.d)
        if on_dev:
            return D, I, R
        return D.cpu().numpy(), I.cpu().numpy(), R.cpu().numpy()

    def make_direct_map(self, new_maintain_direct_map=True):
        """faiss.IndexIVF.make_direct_map: True builds the id -> row map now (Array where every id lies in [0, ntotal) once, else
        Hashtable), False releases it.  Never required: the first reconstruct builds it; every add / remove_ids / reset releases it."""
        _check(lib().rsx_make_direct_map(self._h, DirectMap.Array if new_maintain_direct_map else DirectMap.NoMap))

    def set_direct_map_type(self, type):
        """faiss.IndexIVF.set_direct_map_type(DirectMap.NoMap | Array | Hashtable) (rsx_make_direct_map)."""
        _check(lib().rsx_make_direct_map(self._h, int(type)))

    @property
    def direct_map_type(self):
        """What the handle holds now: DirectMap.NoMap (also: a Flat / IndexPQ handle, whose keys are rows), Array or Hashtable."""
        return self._get("direct_map_type")


class DirectMap:
    """faiss.DirectMap.Type: the map from a stored id to its storage row (rsx_direct_map_type)."""
    NoMap, Array, Hashtable = 0, 1, 2


class InvertedLists:
    """faiss.InvertedLists.subset_type_t: what copy_subset_to selects (rsx_subset_type)."""
    SUBSET_TYPE_ID_RANGE, SUBSET_TYPE_ID_MOD, SUBSET_TYPE_ELEMENT_RANGE, SUBSET_TYPE_INVLIST_FRACTION, SUBSET_TYPE_INVLIST = 0, 1, 2, 3, 4


class IndexFlat(Index):
    def __init__(self, d, metric=METRIC_L2, device=None, devices=None):
        super().__init__(_create(0, d, 1, 0, 8, metric, device, devices), int(d), int(metric))


class IndexFlatIP(IndexFlat):
    def __init__(self, d, device=None, devices=None):
        super().__init__(d, METRIC_INNER_PRODUCT, device, devices)


class IndexFlatL2(IndexFlat):
    def __init__(self, d, device=None, devices=None):
        super().__init__(d, METRIC_L2, device, devices)


class _IndexIVF(Index):
    @property
    def nprobe(self):
        return self._get("nprobe")

    @nprobe.setter
    def nprobe(self, v):
        _check(lib().rsx_set_nprobe(self._h, int(v)))

    @property
    def nlist(self):
        return self._get("nlist")

    def set_centroids(self, c):
        c = np.ascontiguousarray(c, dtype=np.float32)
        assert c.shape == (self.nlist, self.d)
        _check(lib().rsx_set_centroids(self._h, c.ctypes.data_as(ctypes.c_void_p)))

    def get_centroids(self):
        c = np.empty((self.nlist, self.d), dtype=np.float32)
        _check(lib().rsx_get_centroids(self._h, c.ctypes.data_as(ctypes.c_void_p)))
        return c

    def assign(self, x):
        """index.quantizer.assign(x): list number of every vector (exact argmax-IP, as `add` computes it)."""
        keep, p, n, dt, on_dev = _as_matrix(x, self.d, "assign")
        _sync_producer(keep, on_dev)
        labels = np.empty(n, dtype=np.int64)
        _check(lib().rsx_assign(self._h, ctypes.c_int64(n), p, dt, labels.ctypes.data_as(ctypes.c_void_p)))
        return labels

    def reserve_lists(self, counts):
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        assert counts.shape == (self.nlist,)
        _check(lib().rsx_reserve_lists(self._h, counts.ctypes.data_as(ctypes.c_void_p)))

    def copy_subset_to(self, other, subset_type, a1, a2):
        """faiss.IndexIVF.copy_subset_to(other, subset_type, a1, a2): `other` gains the selected entries of every list behind its own, in
        list order and with their ids; this index is unchanged (rsx_copy_subset_to).  subset_type: InvertedLists.SUBSET_TYPE_ID_RANGE
        (a1 <= id < a2), _ID_MOD (id % a1 == a2) or _ELEMENT_RANGE (elements a1 .. a2 - 1 of ntotal, split evenly over the lists)."""
        if not isinstance(other, Index):
            raise TypeError(f"copy_subset_to: the other index must be an rsx index handle, got {type(other).__name__}")
        _check(lib().rsx_copy_subset_to(self._h, other._h, int(subset_type), ctypes.c_int64(int(a1)), ctypes.c_int64(int(a2))))

    def add_list(self, list_no, payload, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if self._get("kind") in (2, 4):
            payload = np.ascontiguousarray(payload, dtype=np.uint8)
            assert payload.ndim == 2 and payload.shape[1] == (self.d if self._get("kind") == 4 else self._get("M")), "add_list: codes of the wrong width"
            dt = _F32
        else:
            payload = np.ascontiguousarray(payload)
            if payload.dtype not in (np.float32, np.float16):
                payload = payload.astype(np.float32)
            dt = _F16 if payload.dtype == np.float16 else _F32
        assert payload.shape[0] == ids.shape[0]
        _check(lib().rsx_add_list(self._h, ctypes.c_int64(list_no), ctypes.c_int64(ids.shape[0]),
                                  payload.ctypes.data_as(ctypes.c_void_p), dt, ids.ctypes.data_as(ctypes.c_void_p)))


def _quantizer_metric(quantizer, metric):
    # The reference passes faiss.IndexFlatIP(d) as the coarse quantiser (ivf_flat.py:143): its
    # metric decides the assignment rule.  The library folds the quantiser into the IVF handle.
    if quantizer is not None and getattr(quantizer, "metric_type", metric) != METRIC_INNER_PRODUCT:
        raise RuntimeError("rsx: only inner-product coarse quantisers are implemented (the reference uses IndexFlatIP)")


class IndexIVFFlat(_IndexIVF):
    def __init__(self, quantizer, d, nlist, metric=METRIC_L2, device=None, devices=None):
        _quantizer_metric(quantizer, metric)
        super().__init__(_create(1, d, nlist, 0, 8, metric, device, devices), int(d), int(metric))
        self.quantizer = quantizer


class IndexIVFPQ(_IndexIVF):
    def __init__(self, quantizer, d, nlist, M, nbits, metric=METRIC_L2, device=None, devices=None):
        _quantizer_metric(quantizer, metric)
        super().__init__(_create(2, d, nlist, M, nbits, metric, device, devices), int(d), int(metric))
        self.quantizer = quantizer
        self.M = int(M)
        self.nbits = int(nbits)

    def set_codebooks(self, cb):
        cb = np.ascontiguousarray(cb, dtype=np.float32)
        assert cb.shape == (self.M, 256, self.d // self.M)
        _check(lib().rsx_set_codebooks(self._h, cb.ctypes.data_as(ctypes.c_void_p)))

    def get_codebooks(self):
        cb = np.empty((self.M, 256, self.d // self.M), dtype=np.float32)
        _check(lib().rsx_get_codebooks(self._h, cb.ctypes.data_as(ctypes.c_void_p)))
        return cb


class ScalarQuantizer:
    """faiss.ScalarQuantizer: the quantiser-type constants, and — as IndexIVFScalarQuantizer.sq — the type and trained parameters of an index."""
    QT_8bit, QT_4bit, QT_8bit_uniform, QT_4bit_uniform, QT_fp16, QT_8bit_direct, QT_6bit = 0, 1, 2, 3, 4, 5, 6

    def __init__(self, index=None):
        self._index = index

    @property
    def qtype(self):
        return self._index._get("qtype")

    @property
    def code_size(self):
        return self._index._get("code_size")

    @property
    def trained(self):
        """float32 [2 d]: vmin[d] then vdiff[d] (faiss ScalarQuantizer::trained for QT_8bit)."""
        t = np.empty(2 * self._index.d, dtype=np.float32)
        _check(lib().rsx_get_sq_trained(self._index._h, t.ctypes.data_as(ctypes.c_void_p)))
        return t


class IndexIVFScalarQuantizer(_IndexIVF):
    """faiss.IndexIVFScalarQuantizer(quantizer, d, nlist, qtype, metric=METRIC_L2, by_residual=True) — factory "IVF<nlist>,SQ8": one code
    byte per dimension in the inverted lists (rsx_ivfsq_create).  Only ScalarQuantizer.QT_8bit.  A search returns the exact
    Flat scores of the queries against the DECODED vectors of the probed lists.  Not in this build (each refused with a message naming the
    kind): selectors / SearchParameters with a selector, remove_ids, sharded handles, the two-call search, IndexRefineFlat over it, FAISS-format files."""

    def __init__(self, quantizer, d, nlist, qtype=ScalarQuantizer.QT_8bit, metric=METRIC_L2, by_residual=True, device=None, devices=None):
        _quantizer_metric(quantizer, metric)
        devs = _resolve_devices(device, devices)
        if devs is not None and len(devs) > 1:
            raise RuntimeError("IndexIVFScalarQuantizer (kind 4) has no sharded form in this build: name one device")
        if devs is not None:
            device = devs[0]
        h = ctypes.c_void_p()
        _check(lib().rsx_ivfsq_create(int(d), int(nlist), int(qtype), int(metric), 1 if by_residual else 0,
                                      default_device() if device is None else int(device), ctypes.byref(h)))
        super().__init__(h, int(d), int(metric))
        self.quantizer = quantizer
        self.sq = ScalarQuantizer(self)

    @property
    def by_residual(self):
        return bool(self._get("by_residual"))

    @property
    def code_size(self):
        return self._get("code_size")

    def set_sq_trained(self, trained):
        """Import the scalar quantiser's parameters (float32 [2 d]: vmin then vdiff), the counterpart of set_codebooks."""
        t = np.ascontiguousarray(trained, dtype=np.float32)
        assert t.shape == (2 * self.d,)
        _check(lib().rsx_set_sq_trained(self._h, t.ctypes.data_as(ctypes.c_void_p)))

    def search_prepass(self, x, k, params=None):
        raise RuntimeError("search_prepass (the two-call search): not available on an IndexIVFScalarQuantizer (kind 4) in this build")


class IndexScalarQuantizer(Index):
    """faiss.IndexScalarQuantizer(d, qtype, metric=METRIC_L2) — factory "SQ8": a flat scalar quantiser, one code byte per dimension and no coarse
    stage: every query scans every code (rsx_sq_create).  Only ScalarQuantizer.QT_8bit.  A search returns the exact Flat scores
    of the queries against the DECODED vectors; batches of more than 32 queries take the certified int8 matrix-core scan.  Sequential ids:
    no add_with_ids (FAISS's IndexFlatCodes has none).  Not in this build (each refused with a message naming the kind): selectors /
    SearchParameters with a selector, remove_ids, range_search, the two-call search, sharded handles, IndexRefineFlat over it, FAISS-format
    files."""

    def __init__(self, d, qtype=ScalarQuantizer.QT_8bit, metric=METRIC_L2, device=None, devices=None):
        devs = _resolve_devices(device, devices)
        if devs is not None and len(devs) > 1:
            raise RuntimeError("IndexScalarQuantizer (kind 5) has no sharded form in this build: name one device")
        if devs is not None:
            device = devs[0]
        h = ctypes.c_void_p()
        _check(lib().rsx_sq_create(int(d), int(qtype), int(metric), default_device() if device is None else int(device), ctypes.byref(h)))
        super().__init__(h, int(d), int(metric))
        self.sq = ScalarQuantizer(self)

    code_size = IndexIVFScalarQuantizer.code_size
    set_sq_trained = IndexIVFScalarQuantizer.set_sq_trained

    def add_with_ids(self, x, ids):
        raise RuntimeError("IndexScalarQuantizer (kind 5): add_with_ids not implemented for this type of index (FAISS's IndexFlatCodes has none)")

    def search_prepass(self, x, k, params=None):
        raise RuntimeError("search_prepass (the two-call search): not available on an IndexScalarQuantizer (kind 5) in this build")

    def range_search(self, x, radius, *, params=None):
        raise RuntimeError("range_search: not available on an IndexScalarQuantizer (kind 5) in this build (IndexFlat* and IndexIVFFlat only)")

    def add_codes(self, codes):
        """Bulk import of already encoded vectors (uint8 [n, d]) behind the stored ones, sequential ids (rsx_add_list, list 0)."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        assert codes.ndim == 2 and codes.shape[1] == self.d
        n0 = self.ntotal
        ids = np.arange(n0, n0 + len(codes), dtype=np.int64)
        if len(codes):
            _check(lib().rsx_add_list(self._h, ctypes.c_int64(0), ctypes.c_int64(len(codes)), codes.ctypes.data_as(ctypes.c_void_p), _F32,
                                      ids.ctypes.data_as(ctypes.c_void_p)))


class IndexPQ(Index):
    """faiss.IndexPQ(d, M, nbits=8, metric=METRIC_L2): a flat product quantiser — no coarse stage, every query scans every code
    (contriever/src/index.py:19, built by passage_retrieval.py --n_subquantizers; rsx_pq_create).  nbits must be 8.  `pq_layout`
    (set_param, before the first add) picks the code layout as for IndexIVFPQ; both metrics take the staged filtered scan in the rotated / sliced layouts (L2 through
    negated per-query tables: the one list's centroid is zero), set_param("pq_fast", 0) switches back to the exact scan.
    No add_with_ids (FAISS's IndexFlatCodes has none), no remove_ids, no search parameters (as FAISS 1.8.0's IndexPQ::search)."""

    def __init__(self, d, M, nbits=8, metric=METRIC_L2, device=None):
        super().__init__(_create(3, d, 1, M, nbits, metric, device, None), int(d), int(metric))
        self.M = int(M)
        self.nbits = int(nbits)

    set_codebooks = IndexIVFPQ.set_codebooks
    get_codebooks = IndexIVFPQ.get_codebooks

    def add_codes(self, codes):
        """Bulk import of already encoded vectors (uint8 [n, M]) behind the stored ones, sequential ids (the FAISS reader's path)."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        assert codes.ndim == 2 and codes.shape[1] == self.M
        n0 = self.ntotal
        ids = np.arange(n0, n0 + len(codes), dtype=np.int64)
        if len(codes):
            _check(lib().rsx_add_list(self._h, ctypes.c_int64(0), ctypes.c_int64(len(codes)), codes.ctypes.data_as(ctypes.c_void_p), _F32,
                                      ids.ctypes.data_as(ctypes.c_void_p)))

    def reconstruct_n(self, i0=0, n=None):
        """Decoded vectors float32 [n, d] of the stored codes i0 .. i0 + n - 1, clipped to ntotal (a slice, as before): the codebook
        entries alone, gathered on the GPU (rsx_reconstruct_batch)."""
        i0 = int(i0)
        hi = self.ntotal if n is None else min(self.ntotal, i0 + int(n))
        return self._reconstruct_keys(np.arange(i0, max(i0, hi), dtype=np.int64), False)


class IndexRefineSearchParameters(SearchParameters):
    """faiss.IndexRefineSearchParameters(k_factor=1, base_index_params=None): k_factor replaces index.k_factor for the call;
    base_index_params (SearchParameters / SearchParametersIVF) goes to the base index's search unchanged."""

    def __init__(self, k_factor=1, base_index_params=None):
        super().__init__(None)
        self.k_factor = k_factor
        self.base_index_params = base_index_params


def refine_k_base(k, k_factor):
    """Candidates IndexRefineFlat asks its base index for: FAISS 1.8.0 IndexRefine::search computes idx_t(k * k_factor) after
    FAISS_THROW_IF_NOT(k_factor >= 1)."""
    if not k_factor >= 1:
        raise AssertionError(f"IndexRefine: k_factor must be >= 1 (FAISS: 'Error: k_factor >= 1 failed'), got {k_factor}")
    return int(int(k) * float(k_factor))


def _has_explicit_ids(index):
    return bool(index._get("explicit_ids"))


class IndexRefineFlat:
    """faiss.IndexRefineFlat(base_index): search the base index for k * k_factor candidates, re-score exactly those against the
    stored vectors (refine_index, an IndexFlat of the base's metric on the base's device) and keep the best k (rsx_refine).
    Bases: any unsharded IndexIVFPQ, IndexPQ, IndexIVFFlat or IndexFlat of sequential ids (a refined label is a row of refine_index).
    As in FAISS's IndexRefine there is no add_with_ids and no remove_ids."""

    def __init__(self, base_index, k_factor=1.0):
        if isinstance(base_index, IndexIVFScalarQuantizer):
            raise RuntimeError("IndexRefineFlat: an IndexIVFScalarQuantizer base (kind 4) is not supported in this build")
        if isinstance(base_index, IndexScalarQuantizer):
            raise RuntimeError("IndexRefineFlat: an IndexScalarQuantizer base (kind 5) is not supported in this build")
        if not isinstance(base_index, (IndexIVFPQ, IndexPQ, IndexIVFFlat, IndexFlat)):
            raise TypeError(f"IndexRefineFlat: the base must be an IndexIVFPQ, IndexPQ, IndexIVFFlat or IndexFlat, got {type(base_index).__name__}")
        if base_index.nshards:
            raise RuntimeError("IndexRefineFlat: a sharded base index is not supported (the refine store lives on one device)")
        if _has_explicit_ids(base_index):
            raise RuntimeError("IndexRefineFlat: the base index holds explicit ids; refined labels are positions of the stored rows")
        self.base_index = base_index
        self.refine_index = IndexFlat(base_index.d, base_index.metric_type, device=base_index._get("device"))
        self.k_factor = float(k_factor)

    @classmethod
    def _from_parts(cls, base_index, refine_index, k_factor):
        if base_index.nshards or refine_index.nshards:
            raise RuntimeError("IndexRefineFlat: sharded parts are not supported")
        if base_index.ntotal != refine_index.ntotal or base_index.d != refine_index.d:
            raise RuntimeError(f"IndexRefineFlat: the base holds {base_index.ntotal} x {base_index.d} vectors, the refine store "
                               f"{refine_index.ntotal} x {refine_index.d}")
        obj = cls.__new__(cls)
        obj.base_index, obj.refine_index, obj.k_factor = base_index, refine_index, float(k_factor)
        return obj

    d = property(lambda self: self.base_index.d)
    metric_type = property(lambda self: self.base_index.metric_type)
    ntotal = property(lambda self: self.base_index.ntotal)
    is_trained = property(lambda self: self.base_index.is_trained)
    nshards = 0

    def train(self, x):
        self.base_index.train(x)

    def add(self, x):
        if _has_explicit_ids(self.base_index):
            raise RuntimeError("IndexRefineFlat.add: the base index holds explicit ids; refined labels are positions of the stored rows")
        if self.base_index.ntotal != self.refine_index.ntotal:
            raise RuntimeError(f"IndexRefineFlat.add: the base holds {self.base_index.ntotal} vectors, the refine store {self.refine_index.ntotal}")
        self.base_index.add(x)
        self.refine_index.add(x)
        assert self.base_index.ntotal == self.refine_index.ntotal, "IndexRefineFlat: the two parts disagree on ntotal after add"

    def reset(self):
        self.base_index.reset()
        self.refine_index.reset()

    def add_with_ids(self, x, ids):
        raise RuntimeError("IndexRefineFlat: add_with_ids not implemented for this type of index (FAISS's IndexRefine has none: "
                           "refined labels are positions in the refine store)")

    def remove_ids(self, x):
        raise RuntimeError("IndexRefineFlat: remove_ids not implemented for this type of index (FAISS's IndexRefine has none)")

    def merge_from(self, other, add_id=0):
        raise RuntimeError("IndexRefineFlat: merge_from not implemented for this type of index (FAISS's IndexRefine has none)")

    def range_search(self, x, radius, *, params=None):
        raise RuntimeError("IndexRefineFlat: range_search is not available in this build (IndexFlat* and IndexIVFFlat only)")

    # faiss.IndexRefine::reconstruct: refine_index's row
    def reconstruct(self, key):
        return self.refine_index.reconstruct(key)

    def reconstruct_batch(self, keys):
        return self.refine_index.reconstruct_batch(keys)

    def reconstruct_n(self, i0=0, n=None):
        return self.refine_index.reconstruct_n(i0, n)

    def make_direct_map(self, new_maintain_direct_map=True):
        self.refine_index.make_direct_map(new_maintain_direct_map)

    def search_and_reconstruct(self, x, k, *, params=None):
        """-> (D, I, R): this index's search, then refine_index's rows of the labels (all-ones words where a label is -1)."""
        on_dev = _is_torch(x) and x.is_cuda
        if on_dev:
            xq = x
        else:
            import torch
            xh = x if _is_torch(x) else np.asarray(x)
            if not _is_torch(xh) and xh.dtype not in (np.float32, np.float16):
                xh = xh.astype(np.float32)
            xq = torch.as_tensor(xh).to(f"cuda:{self.refine_index._get('device')}")
        D, I = self.search(xq, k, params=params)
        R = self.refine_index._reconstruct_keys(I, True).reshape(I.shape[0], I.shape[1], self.d)
        if on_dev:
            return D, I, R
        return D.cpu().numpy(), I.cpu().numpy(), R.cpu().numpy()

    def search(self, x, k, *, params=None):
        """-> (D float32 [n,k], I int64 [n,k]); numpy in -> numpy out, CUDA tensor in -> CUDA tensors out.  The queries are uploaded
        once and the candidate labels stay on the device between the base search and rsx_refine."""
        k = int(k)
        assert k > 0, "k must be positive"
        k_factor, base_params = self.k_factor, None
        if params is not None:
            if not isinstance(params, IndexRefineSearchParameters):
                raise RuntimeError("IndexRefine params have incorrect type")
            k_factor, base_params = params.k_factor, params.base_index_params
        k_base = refine_k_base(k, k_factor)
        if _is_torch(x) and x.is_cuda:
            xq = x
        else:
            import torch
            xh = x if _is_torch(x) else np.asarray(x)
            if not _is_torch(xh) and xh.dtype not in (np.float32, np.float16):
                xh = xh.astype(np.float32)
            xq = torch.as_tensor(xh).to(f"cuda:{self.refine_index._get('device')}")
        _, labels = self.base_index.search(xq, k_base, params=base_params)
        keep, p, n, dt, _ = _as_matrix(xq, self.d, "search")
        import torch
        D = torch.empty((n, k), dtype=torch.float32, device=keep.device)
        I = torch.empty((n, k), dtype=torch.int64, device=keep.device)
        _sync_producer(keep, True)
        _check(lib().rsx_refine(self.refine_index._h, ctypes.c_int64(n), p, dt, k_base, ctypes.c_void_p(labels.data_ptr()), k,
                                ctypes.c_void_p(D.data_ptr()), ctypes.c_void_p(I.data_ptr())))
        if xq is x:
            return D, I
        return D.cpu().numpy(), I.cpu().numpy()


# ------------------------------------------------------------------------------------------
# persistence
# ------------------------------------------------------------------------------------------
def _wrap_handle(h):
    v = ctypes.c_int64(0)

    def g(key):
        _check(lib().rsx_get(h, key.encode(), ctypes.byref(v)))
        return v.value

    kind, d, metric = g("kind"), g("d"), g("metric")
    cls = {0: IndexFlat, 1: IndexIVFFlat, 2: IndexIVFPQ, 3: IndexPQ, 4: IndexIVFScalarQuantizer, 5: IndexScalarQuantizer}[kind]
    obj = cls.__new__(cls)
    Index.__init__(obj, h, d, metric)
    if kind in (2, 3):
        obj.M, obj.nbits = g("M"), g("nbits")
    if kind in (1, 2, 4):
        obj.quantizer = None
    if kind in (4, 5):
        obj.sq = ScalarQuantizer(obj)
    return obj


def write_index(index, path):
    """faiss.write_index(index, path).  Default: the native RSX1 container (magic-tagged; rsx.read_index loads it whatever the
    file is called — the reference's mirrors keep its `index_*.faiss` names).  RSX_INDEX_FORMAT=faiss writes a FAISS-format file
    through rsx_faiss_io instead, for hand-over to a real faiss.read_index (written from upstream knowledge of the format,
    unverified against a FAISS-produced file: DESIGN.md)."""
    if getattr(index, "_is_pretransform", False):
        if os.environ.get("RSX_INDEX_FORMAT", "").lower() == "faiss":
            raise RuntimeError("write_index: an IndexPreTransform has no FAISS-format writer in this build (RSX_INDEX_FORMAT=faiss; FAISS's IxPT / VTrs "
                               "records); unset it to write the native RSXT manifest")
        from rsx_vt import _write_pretransform
        return _write_pretransform(index, os.fspath(path))
    if os.environ.get("RSX_INDEX_FORMAT", "").lower() == "faiss" and index.nshards == 0:
        if isinstance(index, IndexIVFScalarQuantizer):
            raise RuntimeError("write_index: an IndexIVFScalarQuantizer (kind 4) has no FAISS-format writer in this build (RSX_INDEX_FORMAT=faiss); "
                               "unset it to write the native RSX1 container")
        if isinstance(index, IndexScalarQuantizer):
            raise RuntimeError("write_index: an IndexScalarQuantizer (kind 5) has no FAISS-format writer in this build (RSX_INDEX_FORMAT=faiss: "
                               "FAISS's IxSQ record); unset it to write the native RSX1 container")
        from rsx_faiss_io import write_faiss_index
        return write_faiss_index(index, os.fspath(path))
    if isinstance(index, IndexRefineFlat):
        return _write_refine(index, os.fspath(path))
    _check(lib().rsx_save(index._h, os.fspath(path).encode()))


_REFINE_MAGIC = b"RSXR"


def _write_refine(index, path):
    """The RSXR manifest of an IndexRefineFlat: magic | version u32 | k_factor f64 (the Python attribute, exactly; FAISS's IxRF record
    keeps a float32) | two length-prefixed (u32) file names relative to the manifest's directory — the RSX1 files of the base and the
    refine store, written beside it (as the RSXS manifest and its shards)."""
    import struct
    names = [os.path.basename(path) + ".base", os.path.basename(path) + ".refine"]
    here = os.path.dirname(path)
    _check(lib().rsx_save(index.base_index._h, os.path.join(here, names[0]).encode()))
    _check(lib().rsx_save(index.refine_index._h, os.path.join(here, names[1]).encode()))
    with open(path, "wb") as f:
        f.write(_REFINE_MAGIC + struct.pack("<Id", 1, index.k_factor))
        for nm in names:
            b = nm.encode()
            f.write(struct.pack("<I", len(b)) + b)


def _read_refine(path, device):
    import struct
    with open(path, "rb") as f:
        f.read(4)
        version, k_factor = struct.unpack("<Id", f.read(12))
        if version != 1:
            raise RuntimeError(f"{path}: RSXR manifest version {version} is not supported")
        names = []
        for _ in range(2):
            n, = struct.unpack("<I", f.read(4))
            names.append(f.read(n).decode())
    parts = []
    for nm in names:
        h = ctypes.c_void_p()
        _check(lib().rsx_load(os.path.join(os.path.dirname(path), nm).encode(), default_device() if device is None else int(device), ctypes.byref(h)))
        parts.append(_wrap_handle(h))
    return IndexRefineFlat._from_parts(parts[0], parts[1], k_factor)


def read_index(path, device=None, devices=None):
    """faiss.read_index(path): loads an RSX1 container (RSXS: the manifest of a sharded index, one shard per device; RSXR: the
    manifest of an IndexRefineFlat, RSXT: the manifest of an IndexPreTransform, one device only), or a FAISS-format file via rsx_faiss_io.

    A multi-device request (devices=[...] / "all", cfg.datastore.index.devices, RSX_DEVICES) on a file written from ONE
    index — RSX1 or FAISS — RE-SHARDS it while loading: every inverted list / row block is cut over the devices as it
    streams in (ids kept), so an index built on one GPU or handed over from FAISS is served by the whole node and answers
    exactly as before.  (write_index on the result saves the sharded form; the next load is then direct.)"""
    path = os.fspath(path)
    with open(path, "rb") as f:
        magic = f.read(4)
    devs = None if device is not None else _resolve_devices(None, devices)
    multi = devs is not None and len(devs) > 1
    if magic == b"RSXS" or (magic == b"RSX1" and multi):
        devs = devs or [default_device() if device is None else int(device)]
        arr = (ctypes.c_int * len(devs))(*devs)
        h = ctypes.c_void_p()
        _check(lib().rsx_load_sharded(path.encode(), len(devs), arr, ctypes.byref(h)))
        return _wrap_handle(h)
    if device is None and devs:        # a one-entry device list names the device of an ordinary handle
        device = devs[0]
    if magic in (_REFINE_MAGIC, b"IxRF") and multi:
        raise RuntimeError(f"{path}: an IndexRefineFlat cannot be loaded onto several devices (no sharded form)")
    if magic == _REFINE_MAGIC:
        return _read_refine(path, device)
    if magic in (b"RSXT", b"IxPT") and multi:
        raise RuntimeError(f"{path}: an IndexPreTransform cannot be loaded onto several devices (no sharded form)")
    if magic == b"RSXT":
        from rsx_vt import _read_pretransform
        return _read_pretransform(path, device)
    if magic == b"IxPT":
        raise RuntimeError(f"{path}: a FAISS-format IndexPreTransform (IxPT) has no reader in this build; write it with rsx.write_index (RSXT)")
    if magic != b"RSX1":
        from rsx_faiss_io import read_faiss_index
        return read_faiss_index(path, device=device, devices=devs if multi else None)
    h = ctypes.c_void_p()
    _check(lib().rsx_load(path.encode(), default_device() if device is None else int(device), ctypes.byref(h)))
    return _wrap_handle(h)


# ------------------------------------------------------------------------------------------
# multi-shard merge (src/search.py:362-367)
# ------------------------------------------------------------------------------------------
def merge_topk(D, I, metric=METRIC_INNER_PRODUCT, device=None):
    """D, I: [nshards, nq, k] (numpy or CUDA tensors) -> merged (D, I) [nq, k] on the GPU kernel."""
    dev = default_device() if device is None else int(device)
    if _is_torch(D):
        import torch
        D = D.contiguous().float()
        I = I.contiguous().to(torch.int64)
        ns, nq, k = D.shape
        if D.is_cuda:
            Do = torch.empty((nq, k), dtype=torch.float32, device=D.device)
            Io = torch.empty((nq, k), dtype=torch.int64, device=D.device)
            torch.cuda.current_stream(D.device).synchronize()
            _check(lib().rsx_merge_topk(ns, ctypes.c_int64(nq), k, int(metric), ctypes.c_void_p(D.data_ptr()),
                                        ctypes.c_void_p(I.data_ptr()), ctypes.c_void_p(Do.data_ptr()),
                                        ctypes.c_void_p(Io.data_ptr()), D.device.index if D.device.index is not None else dev))
            return Do, Io
        D, I = D.numpy(), I.numpy()
    D = np.ascontiguousarray(D, dtype=np.float32)
    I = np.ascontiguousarray(I, dtype=np.int64)
    ns, nq, k = D.shape
    Do = np.empty((nq, k), dtype=np.float32)
    Io = np.empty((nq, k), dtype=np.int64)
    _check(lib().rsx_merge_topk(ns, ctypes.c_int64(nq), k, int(metric), D.ctypes.data_as(ctypes.c_void_p),
                                I.ctypes.data_as(ctypes.c_void_p), Do.ctypes.data_as(ctypes.c_void_p),
                                Io.ctypes.data_as(ctypes.c_void_p), dev))
    return Do, Io


def pack_topk(D, I, id_offset=0):
    """One rank's CUDA (D, I) [nq, k] -> packed [2, nq, k] int64 (score bits | ids + id_offset) on torch's current stream."""
    import torch
    D = D.contiguous().float(); I = I.contiguous().to(torch.int64)
    nq, k = D.shape
    out = torch.empty((2, nq, k), dtype=torch.int64, device=D.device)
    _check(lib().rsx_pack_topk(ctypes.c_int64(nq), k, ctypes.c_void_p(D.data_ptr()), ctypes.c_void_p(I.data_ptr()),
                               ctypes.c_int64(int(id_offset)), ctypes.c_void_p(out.data_ptr()), D.device.index or 0,
                               ctypes.c_void_p(torch.cuda.current_stream(D.device).cuda_stream)))
    return out


def merge_packed(gathered, metric=METRIC_INNER_PRODUCT):
    """gathered: CUDA int64 [nshards, 2, nq, k] (an all-gather of pack_topk blocks) -> merged (D, I) [nq, k], same rule as
    merge_topk; runs on torch's current stream without a host synchronisation."""
    import torch
    gathered = gathered.contiguous()
    ns, two, nq, k = gathered.shape
    assert two == 2 and gathered.dtype == torch.int64 and gathered.is_cuda
    Do = torch.empty((nq, k), dtype=torch.float32, device=gathered.device)
    Io = torch.empty((nq, k), dtype=torch.int64, device=gathered.device)
    _check(lib().rsx_merge_packed(ns, ctypes.c_int64(nq), k, int(metric), ctypes.c_void_p(gathered.data_ptr()),
                                  ctypes.c_void_p(Do.data_ptr()), ctypes.c_void_p(Io.data_ptr()), gathered.device.index or 0,
                                  ctypes.c_void_p(torch.cuda.current_stream(gathered.device).cuda_stream)))
    return Do, Io


# ------------------------------------------------------------------------------------------
# synthetic data (bench / tests)
# ------------------------------------------------------------------------------------------
def synth_vectors(d, ncentres, seed_c, seed_x, sigma, i0, n, out=None, device=None):
    dev = default_device() if device is None else int(device)
    if out is not None and _is_torch(out):
        _check(lib().rsx_synth_vectors(dev, d, ncentres, ctypes.c_uint32(seed_c), ctypes.c_uint32(seed_x),
                                       ctypes.c_float(sigma), ctypes.c_int64(i0), ctypes.c_int64(n),
                                       ctypes.c_void_p(out.data_ptr())))
        return out
    arr = np.empty((n, d), dtype=np.float16)
    _check(lib().rsx_synth_vectors(dev, d, ncentres, ctypes.c_uint32(seed_c), ctypes.c_uint32(seed_x),
                                   ctypes.c_float(sigma), ctypes.c_int64(i0), ctypes.c_int64(n),
                                   arr.ctypes.data_as(ctypes.c_void_p)))
    return arr


def synth_queries(d, ncentres, seed_c, seed_x, sigma, nbase, seed_q, sigma_q, r0, n, out=None, device=None):
    dev = default_device() if device is None else int(device)
    if out is not None and _is_torch(out):
        _check(lib().rsx_synth_queries(dev, d, ncentres, ctypes.c_uint32(seed_c), ctypes.c_uint32(seed_x),
                                       ctypes.c_float(sigma), ctypes.c_int64(nbase), ctypes.c_uint32(seed_q),
                                       ctypes.c_float(sigma_q), ctypes.c_int64(r0), ctypes.c_int64(n),
                                       ctypes.c_void_p(out.data_ptr())))
        return out
    arr = np.empty((n, d), dtype=np.float16)
    _check(lib().rsx_synth_queries(dev, d, ncentres, ctypes.c_uint32(seed_c), ctypes.c_uint32(seed_x),
                                   ctypes.c_float(sigma), ctypes.c_int64(nbase), ctypes.c_uint32(seed_q),
                                   ctypes.c_float(sigma_q), ctypes.c_int64(r0), ctypes.c_int64(n),
                                   arr.ctypes.data_as(ctypes.c_void_p)))
    return arr


# ------------------------------------------------------------------------------------------
# CUDA-era shims the reference's training branch touches (ivf_flat.py:152-163)
# ------------------------------------------------------------------------------------------
class StandardGpuResources:
    """faiss.StandardGpuResources(): nothing to hold — librsx owns its HBM per index handle."""


class GpuClonerOptions:
    useFloat16 = False


def index_cpu_to_gpu(res, device, index, co=None):
    """The index is already resident on the MI355X; training runs there (rsx_train)."""
    return index


def index_gpu_to_cpu(index):
    return index


# ------------------------------------------------------------------------------------------
# vector transforms, IndexPreTransform, index_factory: module rsx_vt, written against the names above and re-exported here on first use
# (PEP 562), so that either module can be imported first
# ------------------------------------------------------------------------------------------
def __getattr__(name):
    import rsx_vt
    if name in rsx_vt.__all__:
        return getattr(rsx_vt, name)
    raise AttributeError(f"module 'rsx' has no attribute {name!r}")
