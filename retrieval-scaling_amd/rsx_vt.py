"""rsx_vt — the vector transforms and IndexPreTransform of the `rsx` surface (FAISS 1.8.0 names and defaults).

    faiss.VectorTransform / LinearTransform / RandomRotationMatrix / PCAMatrix / OPQMatrix      same names
    faiss.IndexPreTransform(ltrans, index) / SearchParametersPreTransform                         same names
    faiss.index_factory(d, "OPQ96,IVF4096,PQ96") / extract_index_ivf / downcast_index             same names

`rsx` re-exports every public name of this module (rsx.IndexPreTransform, ...).  The transform itself, Y = X·Aᵀ + b, is
k_vt_apply in the HIP library (rsx_vt_apply): one sequential fp32 fmaf chain per output, bit for bit reproducible, so a search
through a transform EQUALS the search of the transformed data.  Training (PCA, OPQ) is plumbing: fp64 sums on the GPU through
torch, the d x d decompositions on the host in numpy fp64.
"""
import ctypes
import os
import re
import struct

import numpy as np

import rsx as _r

__all__ = ["VectorTransform", "LinearTransform", "RandomRotationMatrix", "PCAMatrix", "OPQMatrix", "IndexPreTransform",
           "SearchParametersPreTransform", "index_factory", "parse_index_factory", "extract_index_ivf", "downcast_index",
           "pack_vt_record", "unpack_vt_record"]

F32 = np.float32


def _to_device(x, device):
    """numpy / CPU tensor (fp16 or fp32 kept, anything else -> fp32) -> CUDA tensor on `device`; a CUDA tensor as it is."""
    import torch
    if _r._is_torch(x):
        if x.dtype not in (torch.float32, torch.float16):
            x = x.float()
        return x if x.is_cuda else x.to(f"cuda:{device}")
    x = np.asarray(x)
    if x.dtype not in (np.float32, np.float16):
        x = x.astype(np.float32)
    return torch.as_tensor(np.ascontiguousarray(x)).to(f"cuda:{device}")


def _is_host(x):
    return not (_r._is_torch(x) and x.is_cuda)


def _like_input(x, *outs):
    """CUDA results -> what the caller handed in: numpy for numpy, CPU tensors for a CPU tensor, CUDA tensors as they are."""
    if _r._is_torch(x):
        return outs if x.is_cuda else tuple(o.cpu() for o in outs)
    return tuple(o.cpu().numpy() for o in outs)


# ------------------------------------------------------------------------------------------
# transforms
# ------------------------------------------------------------------------------------------
class VectorTransform:
    """faiss.VectorTransform: d_in, d_out, is_trained, train(x), apply(x), reverse_transform(y)."""

    def __init__(self, d_in=0, d_out=0):
        self.d_in, self.d_out = int(d_in), int(d_out)
        self.is_trained = True

    def train(self, x):
        """Nothing to train by default."""

    def apply(self, x):
        raise NotImplementedError

    def apply_py(self, x):
        """FAISS's Python alias of apply."""
        return self.apply(x)

    def reverse_transform(self, y):
        raise RuntimeError("reverse transform not implemented")


class LinearTransform(VectorTransform):
    """faiss.LinearTransform(d_in, d_out, have_bias=False): y = A·x + b.  A float32 [d_out, d_in], b float32 [d_out] (empty without
    bias).  As in FAISS the object is not trained until a subclass's train() has run or the caller, having ASSIGNED A (and b), sets
    is_trained = True; assign whole arrays — a change made inside the array in place does not reach the GPU copy.  apply():
    numpy in -> numpy float32 out, CUDA tensor in -> CUDA tensor out; fp16 and fp32 inputs are read as they are (rsx_vt_apply:
    y_j = fp32(fmaf chain over t + b_j))."""

    def __init__(self, d_in=0, d_out=0, have_bias=False, device=None):
        super().__init__(d_in, d_out)
        self.have_bias = bool(have_bias)
        self.is_orthonormal = False
        self.is_trained = False
        self.verbose = False
        self._A = np.zeros((0, 0), dtype=F32)
        self._b = np.zeros((0,), dtype=F32)
        self._dirty = True
        self._h = None
        self.device = _r.default_device() if device is None else int(device)
        h = ctypes.c_void_p()
        _r._check(_r.lib().rsx_vt_create(self.device, self.d_in, self.d_out, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _r._lib is not None:
            try:
                _r._lib.rsx_vt_destroy(h)
            except Exception:
                pass
            self._h = None

    @property
    def A(self):
        return self._A

    @A.setter
    def A(self, v):
        self._A = np.ascontiguousarray(v, dtype=F32)
        self._dirty = True

    @property
    def b(self):
        return self._b

    @b.setter
    def b(self, v):
        self._b = np.ascontiguousarray(v, dtype=F32).reshape(-1)
        self._dirty = True

    def _upload(self):
        if not self.is_trained:
            raise RuntimeError(f"{type(self).__name__}: Transformation not trained yet")
        if not self._dirty:
            return
        if self._A.shape != (self.d_out, self.d_in):
            raise RuntimeError(f"{type(self).__name__}: A has shape {self._A.shape}, expected ({self.d_out}, {self.d_in})")
        bp = None
        if self.have_bias:
            if self._b.shape != (self.d_out,):
                raise RuntimeError(f"{type(self).__name__}: have_bias is set and b has shape {self._b.shape}, expected ({self.d_out},)")
            bp = self._b.ctypes.data_as(ctypes.c_void_p)
        _r._check(_r.lib().rsx_vt_set(self._h, self._A.ctypes.data_as(ctypes.c_void_p), bp))
        self._dirty = False

    def _run(self, x, d_from, d_to, reverse, what):
        self._upload()
        keep, p, n, dt, on_dev = _r._as_matrix(x, d_from, what)
        if on_dev:
            import torch
            if keep.device.index != self.device:
                raise RuntimeError(f"{type(self).__name__}.{what}: the tensor lives on {keep.device}, the transform on cuda:{self.device}")
            y = torch.empty((n, d_to), dtype=torch.float32, device=keep.device)
            _r._sync_producer(keep, True)
            _r._check(_r.lib().rsx_vt_apply(self._h, ctypes.c_int64(n), p if n else None, dt, ctypes.c_void_p(y.data_ptr()) if n else None, reverse))
            return y
        y = np.empty((n, d_to), dtype=F32)
        _r._check(_r.lib().rsx_vt_apply(self._h, ctypes.c_int64(n), p if n else None, dt, y.ctypes.data_as(ctypes.c_void_p) if n else None, reverse))
        if _r._is_torch(x):
            import torch
            return torch.from_numpy(y)
        return y

    def apply(self, x):
        return self._run(x, self.d_in, self.d_out, 0, "apply")

    def reverse_transform(self, y):
        """x = Aᵀ·(y - b), FAISS's transform_transpose: the inverse only of an orthonormal A, refused otherwise."""
        if not self.is_orthonormal:
            raise RuntimeError("reverse transform not implemented for non-orthonormal matrices")
        return self._run(y, self.d_out, self.d_in, 1, "reverse_transform")

    def set_is_orthonormal(self):
        """FAISS's rule: orthonormal when every entry of A·Aᵀ - I is at most 4e-5 in magnitude (computed in fp64 here); never when
        d_out > d_in."""
        if self.d_out > self.d_in:
            self.is_orthonormal = False
        elif self.d_out == 0:
            self.is_orthonormal = True
        else:
            A = self._A.astype(np.float64)
            self.is_orthonormal = bool(np.abs(A @ A.T - np.eye(self.d_out)).max() <= 4e-5)
        return self.is_orthonormal

    # -- RSXT record (pack_vt_record)
    _TAG = "LTra"

    def _record(self):
        return {"tag": self._TAG, "d_in": self.d_in, "d_out": self.d_out, "have_bias": self.have_bias, "is_orthonormal": bool(self.is_orthonormal),
                "is_trained": bool(self.is_trained), "A": self._A, "b": self._b, "extra": self._extra()}

    def _extra(self):
        return {}

    def _set_extra(self, extra):
        pass


def _orthonormal_rows(d_in, d_out, seed):
    """float64 [d_out, d_in]: QR of a numpy.random.RandomState(seed) normal matrix, the factor's signs fixed by R's diagonal > 0.
    d_out <= d_in: orthonormal rows; d_out > d_in: orthonormal columns (FAISS keeps d_in columns of a d_out x d_out rotation)."""
    lo, hi = min(d_in, d_out), max(d_in, d_out)
    g = np.random.RandomState(seed).randn(hi, lo)
    q, r = np.linalg.qr(g)
    q = q * np.where(np.diag(r) < 0, -1.0, 1.0)[None, :]
    return q.T if d_out <= d_in else q


class RandomRotationMatrix(LinearTransform):
    """faiss.RandomRotationMatrix(d_in, d_out): a random orthonormal matrix.  init(seed): a numpy.random.RandomState(seed) normal matrix,
    QR in fp64 on the host, rounded once to fp32; train() calls init(12345) when init has not run.  FAISS's own random generator is NOT
    reproduced (the oracle is unpinned: no FAISS build to compare with), so the matrix of a seed differs from FAISS's for that seed."""
    _TAG = "RRot"

    def __init__(self, d_in=0, d_out=0, device=None):
        super().__init__(d_in, d_out, False, device)

    def init(self, seed):
        self.A = _orthonormal_rows(self.d_in, self.d_out, int(seed)).astype(F32)
        self.is_orthonormal = True
        self.is_trained = True

    def train(self, x):
        if not self.is_trained:
            self.init(12345)


def _fp64_moments(t, chunk=1 << 16):
    """CUDA tensor [n, d] -> (mean [d], covariance [d, d] = Σ (x - mean)(x - mean)ᵀ / n), float64 numpy, summed on the GPU."""
    import torch
    n, d = t.shape
    s = torch.zeros(d, dtype=torch.float64, device=t.device)
    for i in range(0, n, chunk):
        s += t[i:i + chunk].double().sum(0)
    mean = s / n
    cov = torch.zeros((d, d), dtype=torch.float64, device=t.device)
    for i in range(0, n, chunk):
        c = t[i:i + chunk].double() - mean
        cov += c.T @ c
    return mean.cpu().numpy(), (cov / n).cpu().numpy()


class PCAMatrix(LinearTransform):
    """faiss.PCAMatrix(d_in, d_out, eigen_power=0, random_rotation=False).  train(x): mean and covariance (Σ(x - mean)(x - mean)ᵀ / n) in
    fp64 on the GPU over ALL rows — no subsampling of the training set (FAISS caps it at max_points_per_d x d_in) — numpy eigh in fp64
    on the host; row j of A = the eigenvector of the j-th largest eigenvalue, signed so that its largest-magnitude component is positive,
    scaled by eigenvalue_j ** eigen_power when eigen_power != 0 (whitening at -0.5: the transform is then not orthonormal and has no
    reverse); random_rotation multiplies a seeded random rotation of the d_out outputs in front, in fp64 (FAISS's seed 5, this module's
    generator).  b = -A·mean (fp64 sum of the fp32 A and the fp32 mean, rounded once).  Attributes: mean float32 [d_in], eigenvalues
    float64 [d_in] descending (FAISS: float32), PCAMat float32 [d_in, d_in] (rows = all eigenvectors, signed)."""
    _TAG = "PCAm"

    def __init__(self, d_in=0, d_out=0, eigen_power=0, random_rotation=False, device=None):
        if d_out > d_in:
            raise RuntimeError(f"PCAMatrix: d_out = {d_out} exceeds d_in = {d_in}")
        super().__init__(d_in, d_out, True, device)
        self.eigen_power = float(eigen_power)
        self.random_rotation = bool(random_rotation)
        self.mean = np.zeros((0,), dtype=F32)
        self.eigenvalues = np.zeros((0,), dtype=np.float64)
        self.PCAMat = np.zeros((0, 0), dtype=F32)

    def train(self, x):
        t = _to_device(x, self.device)
        if t.dim() != 2 or t.shape[1] != self.d_in:
            raise AssertionError(f"PCAMatrix.train: expected shape [n, {self.d_in}], got {tuple(t.shape)}")
        if t.shape[0] < 2:
            raise RuntimeError("PCAMatrix.train: at least two training vectors are needed")
        mean, cov = _fp64_moments(t)
        self.mean = mean.astype(F32)
        w, v = np.linalg.eigh(cov)
        order = np.argsort(-w, kind="stable")
        w, v = w[order], v[:, order].T                    # rows = eigenvectors, largest eigenvalue first
        big = np.abs(v).argmax(axis=1)
        v = v * np.where(v[np.arange(len(v)), big] < 0, -1.0, 1.0)[:, None]
        self.eigenvalues = w
        self.PCAMat = v.astype(F32)
        self.prepare_Ab()
        self.is_trained = True

    def prepare_Ab(self):
        """A and b from PCAMat, eigenvalues, mean, eigen_power and random_rotation (faiss.PCAMatrix::prepare_Ab)."""
        A = self.PCAMat[:self.d_out].astype(np.float64)
        if self.eigen_power != 0:
            A = A * (self.eigenvalues[:self.d_out] ** self.eigen_power)[:, None]
        if self.random_rotation:
            A = _orthonormal_rows(self.d_out, self.d_out, 5) @ A
        self.A = A.astype(F32)
        self.b = (-(self._A.astype(np.float64) @ self.mean.astype(np.float64))).astype(F32)
        self.is_orthonormal = self.eigen_power == 0

    def _extra(self):
        return {"eigen_power": self.eigen_power, "random_rotation": self.random_rotation, "mean": self.mean, "eigenvalues": self.eigenvalues,
                "PCAMat": self.PCAMat}

    def _set_extra(self, e):
        self.eigen_power, self.random_rotation = float(e["eigen_power"]), bool(e["random_rotation"])
        self.mean, self.eigenvalues, self.PCAMat = e["mean"], e["eigenvalues"], e["PCAMat"]


class OPQMatrix(LinearTransform):
    """faiss.OPQMatrix(d, M, d2=-1): the rotation that minimises a product quantiser's error (Ge et al., non-parametric OPQ); niter = 50,
    max_train_points = 65536, verbose.  train(x) alternates, from a seeded random orthonormal d2 x d matrix (seed 1234): rotate the sample
    (k_vt_apply), train a product quantiser on it through a temporary rsx.IndexPQ(d2, M, 8) — train, add, reconstruct_n: the decoded
    sample X^ — form Xᵀ·X^ (d x d2) in fp64 on the GPU, take its SVD U S Vᵀ on the host in fp64 and set A = (U Vᵀ)ᵀ rounded once to fp32.
    DIFFERENCES FROM FAISS: the quantiser is trained by the library's own PQ training as it is in every iteration (FAISS warm-starts it
    with niter_pq = 4 iterations: there is no such attribute here); the sample is not centred; a training set larger than
    max_train_points is cut to a numpy.random.RandomState(1234) subset in row order; d2 > d is refused."""
    _TAG = "OPQm"

    def __init__(self, d=0, M=1, d2=-1, device=None):
        d2 = d if d2 is None or d2 < 0 else int(d2)
        if d2 > d:
            raise RuntimeError(f"OPQMatrix: d2 = {d2} > d = {d} is not supported in this build")
        if M <= 0 or d2 % M:
            raise RuntimeError(f"OPQMatrix: d2 = {d2} is not a multiple of M = {M}")
        super().__init__(d, d2, False, device)
        self.M = int(M)
        self.niter = 50
        self.max_train_points = 256 * 256
        self.pq_errors = []         # mean squared quantisation error of the rotated sample, per iteration

    def train(self, x):
        import torch
        t = _to_device(x, self.device)
        if t.dim() != 2 or t.shape[1] != self.d_in:
            raise AssertionError(f"OPQMatrix.train: expected shape [n, {self.d_in}], got {tuple(t.shape)}")
        n = t.shape[0]
        if n > self.max_train_points:
            keep = np.sort(np.random.RandomState(1234).choice(n, self.max_train_points, replace=False))
            t = t[torch.as_tensor(keep, device=t.device)]
            n = t.shape[0]
        t = t.contiguous()
        keys = torch.arange(n, dtype=torch.int64, device=t.device)
        self.A = _orthonormal_rows(self.d_in, self.d_out, 1234).astype(F32)
        self.is_trained = True           # (apply() below needs it; the matrix is a valid rotation at every point of the loop)
        self.is_orthonormal = True
        self.pq_errors = []
        for it in range(int(self.niter)):
            xr = self.apply(t)
            pq = _r.IndexPQ(self.d_out, self.M, 8, device=self.device)
            pq.train(xr)
            pq.add(xr)
            xhat = pq.reconstruct_batch(keys)
            del pq
            err = float(((xr.double() - xhat.double()) ** 2).sum(1).mean())
            self.pq_errors.append(err)
            if self.verbose:
                print(f"OPQMatrix.train: iteration {it} of {self.niter}: quantisation error {err:.6g}")
            c = torch.zeros((self.d_in, self.d_out), dtype=torch.float64, device=t.device)
            for i in range(0, n, 1 << 16):
                c += t[i:i + (1 << 16)].double().T @ xhat[i:i + (1 << 16)].double()
            u, _, vt = np.linalg.svd(c.cpu().numpy(), full_matrices=False)
            self.A = (u @ vt).T.astype(F32)

    def _extra(self):
        return {"M": self.M, "niter": int(self.niter), "max_train_points": int(self.max_train_points)}

    def _set_extra(self, e):
        self.M, self.niter, self.max_train_points = e["M"], e["niter"], e["max_train_points"]


# ------------------------------------------------------------------------------------------
# RSXT records: one transform as bytes (write_index / read_index of an IndexPreTransform).  Pure functions of plain values.
# ------------------------------------------------------------------------------------------
_TAGS = ("LTra", "RRot", "PCAm", "OPQm")


def _pack_array(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return struct.pack("<I", a.ndim) + struct.pack(f"<{a.ndim}q", *a.shape) + a.tobytes()


def _unpack_array(buf, off, dtype):
    ndim, = struct.unpack_from("<I", buf, off)
    off += 4
    shape = struct.unpack_from(f"<{ndim}q", buf, off)
    off += 8 * ndim
    count = int(np.prod(shape, dtype=np.int64)) if ndim else 1
    nbytes = count * np.dtype(dtype).itemsize
    if off + nbytes > len(buf):
        raise RuntimeError("RSXT: truncated transform record")
    a = np.frombuffer(buf, dtype=dtype, count=count, offset=off).reshape(shape).copy()
    return a, off + nbytes


def pack_vt_record(rec):
    """rec: {"tag", "d_in", "d_out", "have_bias", "is_orthonormal", "is_trained", "A", "b", "extra"} -> bytes:
    tag[4] | d_in i32 | d_out i32 | have_bias, is_orthonormal, is_trained u8 | A f32 array | b f32 array | the kind's own fields
    (PCAm: eigen_power f64, random_rotation u8, mean f32, eigenvalues f64, PCAMat f32; OPQm: M, niter, max_train_points i32).
    An array is ndim u32 | shape i64[ndim] | the values."""
    tag = rec["tag"]
    if tag not in _TAGS:
        raise RuntimeError(f"RSXT: unknown transform kind {tag!r}")
    out = [tag.encode(), struct.pack("<iiBBB", rec["d_in"], rec["d_out"], int(rec["have_bias"]), int(rec["is_orthonormal"]), int(rec["is_trained"])),
           _pack_array(rec["A"], F32), _pack_array(rec["b"], F32)]
    e = rec.get("extra") or {}
    if tag == "PCAm":
        out += [struct.pack("<dB", e["eigen_power"], int(e["random_rotation"])), _pack_array(e["mean"], F32),
                _pack_array(e["eigenvalues"], np.float64), _pack_array(e["PCAMat"], F32)]
    elif tag == "OPQm":
        out.append(struct.pack("<iii", e["M"], e["niter"], e["max_train_points"]))
    return b"".join(out)


def unpack_vt_record(buf, off=0):
    """-> (rec, offset behind the record): the inverse of pack_vt_record."""
    if off + 15 > len(buf):
        raise RuntimeError("RSXT: truncated transform record")
    tag = bytes(buf[off:off + 4]).decode("latin-1")
    if tag not in _TAGS:
        raise RuntimeError(f"RSXT: unknown transform kind {tag!r}")
    d_in, d_out, hb, ortho, trained = struct.unpack_from("<iiBBB", buf, off + 4)
    off += 15
    A, off = _unpack_array(buf, off, F32)
    b, off = _unpack_array(buf, off, F32)
    e = {}
    if tag == "PCAm":
        e["eigen_power"], rr = struct.unpack_from("<dB", buf, off)
        e["random_rotation"] = bool(rr)
        off += 9
        e["mean"], off = _unpack_array(buf, off, F32)
        e["eigenvalues"], off = _unpack_array(buf, off, np.float64)
        e["PCAMat"], off = _unpack_array(buf, off, F32)
    elif tag == "OPQm":
        e["M"], e["niter"], e["max_train_points"] = struct.unpack_from("<iii", buf, off)
        off += 12
    return {"tag": tag, "d_in": d_in, "d_out": d_out, "have_bias": bool(hb), "is_orthonormal": bool(ortho), "is_trained": bool(trained),
            "A": A, "b": b, "extra": e}, off


def _vt_from_record(rec, device):
    tag, d_in, d_out = rec["tag"], rec["d_in"], rec["d_out"]
    if tag == "RRot":
        vt = RandomRotationMatrix(d_in, d_out, device=device)
    elif tag == "PCAm":
        vt = PCAMatrix(d_in, d_out, device=device)
    elif tag == "OPQm":
        vt = OPQMatrix(d_in, rec["extra"]["M"], d_out, device=device)
    else:
        vt = LinearTransform(d_in, d_out, rec["have_bias"], device=device)
    vt.have_bias = rec["have_bias"]
    vt._set_extra(rec["extra"])
    vt.A, vt.b = rec["A"], rec["b"]
    vt.is_orthonormal, vt.is_trained = rec["is_orthonormal"], rec["is_trained"]
    return vt


# ------------------------------------------------------------------------------------------
# IndexPreTransform
# ------------------------------------------------------------------------------------------
class SearchParametersPreTransform(_r.SearchParameters):
    """faiss.SearchParametersPreTransform(index_params=None): index_params goes to the wrapped index's search unchanged — an id selector
    in it selects ids, not coordinates, and needs no transform."""

    def __init__(self, index_params=None):
        super().__init__(None)
        self.index_params = index_params


class IndexPreTransform:
    """faiss.IndexPreTransform(index) / IndexPreTransform(ltrans, index): every vector goes through `chain` (applied first to last, on the
    GPU) before it reaches `index` — an unsharded IndexIVFPQ, IndexPQ, IndexIVFScalarQuantizer, IndexScalarQuantizer, IndexIVFFlat or IndexFlat.  What the
    index accepts and refuses (selectors, range_search, remove_ids, add_with_ids, ...) applies unchanged.  Rotated vectors are not
    fp16-representable: a Flat or IVF-Flat base behind a transform stores fp32 rows (its widened path).  reconstruct* return the index's
    stored vector taken back through the chain, which needs every transform to be orthonormal.  IndexRefineFlat does not take an
    IndexPreTransform as its base in this build."""

    _is_pretransform = True         # (rsx.write_index tells the manifest kinds apart without importing this module)
    add_chunk_rows = 1 << 18        # add: rows transformed per pass (the transformed chunk is a device buffer of add_chunk_rows x d_out floats)

    def __init__(self, *args):
        if len(args) == 1:
            ltrans, index = None, args[0]
        elif len(args) == 2:
            ltrans, index = args
        else:
            raise TypeError("IndexPreTransform(index) or IndexPreTransform(ltrans, index)")
        if not isinstance(index, _r.Index):
            raise TypeError(f"IndexPreTransform: the index must be an IndexIVFPQ, IndexPQ, IndexIVFScalarQuantizer, IndexScalarQuantizer, IndexIVFFlat or IndexFlat, "
                            f"got {type(index).__name__}")
        if index.nshards:
            raise RuntimeError("IndexPreTransform: a sharded index is not supported (the transform lives on one device)")
        self.index = index
        self.chain = []
        if ltrans is not None:
            self.prepend_transform(ltrans)

    def prepend_transform(self, vt):
        if not isinstance(vt, VectorTransform):
            raise TypeError(f"IndexPreTransform: a transform must be a VectorTransform, got {type(vt).__name__}")
        if vt.d_out != self.d:
            raise RuntimeError(f"IndexPreTransform: the transform's d_out = {vt.d_out} does not meet the dimension {self.d} of what follows it")
        dev = self.index._get("device")
        if getattr(vt, "device", dev) != dev:
            raise RuntimeError(f"IndexPreTransform: the transform lives on device {vt.device}, the index on device {dev}")
        self.chain.insert(0, vt)

    d = property(lambda self: self.chain[0].d_in if self.chain else self.index.d)
    ntotal = property(lambda self: self.index.ntotal)
    metric_type = property(lambda self: self.index.metric_type)
    is_trained = property(lambda self: all(vt.is_trained for vt in self.chain) and self.index.is_trained)

    def _dev(self, x, what):
        t = _to_device(x, self.index._get("device"))
        if t.dim() != 2 or t.shape[1] != self.d:
            raise AssertionError(f"{what}: expected shape [n, {self.d}], got {tuple(t.shape)}")
        return t

    def apply_chain(self, x):
        for vt in self.chain:
            x = vt.apply(x)
        return x

    def reverse_chain(self, y):
        for vt in reversed(self.chain):
            y = vt.reverse_transform(y)
        return y

    def train(self, x):
        """Trains each untrained transform on the data as transformed so far, then the index (if untrained) on the fully transformed set."""
        t = self._dev(x, "train")
        for vt in self.chain:
            if not vt.is_trained:
                vt.train(t)
            t = vt.apply(t)
        if not self.index.is_trained:
            self.index.train(t)

    def _add(self, x, ids, what):
        if not self.is_trained:
            raise RuntimeError(f"IndexPreTransform.{what}: the index is not trained")
        if ids is not None:
            ids = np.ascontiguousarray(ids.detach().cpu().numpy() if _r._is_torch(ids) else ids, dtype=np.int64)
        host = _is_host(x)
        if host:
            x = x if _r._is_torch(x) else np.asarray(x)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise AssertionError(f"{what}: expected shape [n, {self.d}], got {tuple(x.shape)}")
        n = x.shape[0]
        if ids is not None and ids.shape != (n,):
            raise AssertionError("ids must have one entry per vector")
        step = max(1, int(self.add_chunk_rows))
        for i in range(0, n, step):
            t = self.apply_chain(self._dev(x[i:i + step], what))
            if ids is None:
                self.index.add(t)
            else:
                self.index.add_with_ids(t, ids[i:i + step])
            del t

    def add(self, x):
        """In chunks of add_chunk_rows rows: upload (a host array), transform, add.  Order and sequential ids are those of one add."""
        self._add(x, None, "add")

    def add_with_ids(self, x, ids):
        self._add(x, ids, "add_with_ids")

    def reset(self):
        self.index.reset()

    def remove_ids(self, x):
        return self.index.remove_ids(x)

    def merge_from(self, other, add_id=0):
        """faiss.IndexPreTransform.merge_from: forwards to the base index when both chains are bit-equal (the same transform kinds and
        matrices); otherwise refused, with both indexes untouched."""
        if not isinstance(other, IndexPreTransform):
            raise RuntimeError(f"IndexPreTransform.merge_from: the other index must be an IndexPreTransform, got {type(other).__name__}")
        if other is self:
            raise RuntimeError("IndexPreTransform.merge_from: source and destination are the same index")
        if len(self.chain) != len(other.chain):
            raise RuntimeError(f"IndexPreTransform.merge_from: the chains differ in length ({len(self.chain)} and {len(other.chain)})")
        for i, (a, b) in enumerate(zip(self.chain, other.chain)):
            ra, rb = a._record(), b._record()
            same = type(a) is type(b) and (ra["d_in"], ra["d_out"], bool(ra["have_bias"])) == (rb["d_in"], rb["d_out"], bool(rb["have_bias"]))
            same = same and all(_pack_array(ra[key], F32) == _pack_array(rb[key], F32) for key in ("A", "b"))
            if not same:
                raise RuntimeError(f"IndexPreTransform.merge_from: transform {i} of the chains differs (kinds and matrices must be bit-equal)")
        self.index.merge_from(other.index, add_id)

    def _index_params(self, params):
        if params is None:
            return None
        if not isinstance(params, SearchParametersPreTransform):
            raise RuntimeError(f"IndexPreTransform params have incorrect type: expected SearchParametersPreTransform, got {type(params).__name__}")
        return params.index_params

    def search(self, x, k, params=None):
        """-> (D, I): the index's search of the transformed queries.  numpy in -> numpy out, CUDA tensor in -> CUDA tensors out."""
        ip = self._index_params(params)
        t = self.apply_chain(self._dev(x, "search"))
        D, I = self.index.search(t, k) if ip is None else self.index.search(t, k, params=ip)
        return _like_input(x, D, I)

    def range_search(self, x, radius, params=None):
        ip = self._index_params(params)
        t = self.apply_chain(self._dev(x, "range_search"))
        out = self.index.range_search(t, radius) if ip is None else self.index.range_search(t, radius, params=ip)
        return _like_input(x, *out)

    def reconstruct_batch(self, keys):
        return self.reverse_chain(self.index.reconstruct_batch(keys))

    def reconstruct(self, key):
        return self.reverse_chain(self.index.reconstruct_batch(np.array([int(key)], dtype=np.int64)))[0]

    def reconstruct_n(self, i0=0, n=None):
        return self.reverse_chain(self.index.reconstruct_n(i0, n))

    def search_and_reconstruct(self, x, k, params=None):
        """-> (D, I, R [n, k, d]): R[i, j] = reconstruct(I[i, j]); every bit of R[i, j] is set where I[i, j] = -1."""
        import torch
        ip = self._index_params(params)
        t = self.apply_chain(self._dev(x, "search_and_reconstruct"))
        D, I, R = self.index.search_and_reconstruct(t, k, params=ip)
        R = self.reverse_chain(R.reshape(-1, R.shape[-1]).contiguous()).reshape(I.shape[0], I.shape[1], self.d)
        R.view(torch.int32)[I < 0] = -1
        return _like_input(x, D, I, R)


_PT_MAGIC = b"RSXT"


def _write_pretransform(index, path):
    """The RSXT manifest: magic | version u32 | number of transforms u32 | their records first to last (pack_vt_record) | the length-prefixed
    (u32) name, relative to the manifest's directory, of the wrapped index's own file, written beside it (as RSXR does)."""
    name = os.path.basename(path) + ".index"
    _r.write_index(index.index, os.path.join(os.path.dirname(path), name))
    with open(path, "wb") as f:
        f.write(_PT_MAGIC + struct.pack("<II", 1, len(index.chain)))
        for vt in index.chain:
            if not isinstance(vt, LinearTransform):
                raise RuntimeError(f"write_index: no RSXT record for a {type(vt).__name__}")
            f.write(pack_vt_record(vt._record()))
        b = name.encode()
        f.write(struct.pack("<I", len(b)) + b)


def _read_pretransform(path, device):
    buf = open(path, "rb").read()
    version, nvt = struct.unpack_from("<II", buf, 4)
    if version != 1:
        raise RuntimeError(f"{path}: RSXT manifest version {version} is not supported")
    off, recs = 12, []
    for _ in range(nvt):
        rec, off = unpack_vt_record(buf, off)
        recs.append(rec)
    n, = struct.unpack_from("<I", buf, off)
    name = buf[off + 4:off + 4 + n].decode()
    base = _r.read_index(os.path.join(os.path.dirname(path), name), device=device)
    dev = base._get("device")
    pt = IndexPreTransform(base)
    for rec in reversed(recs):
        pt.prepend_transform(_vt_from_record(rec, dev))
    return pt


# ------------------------------------------------------------------------------------------
# index_factory
# ------------------------------------------------------------------------------------------
def parse_index_factory(d, description):
    """The factory string as plain values (no GPU): {"transforms": [(kind, args...)], "d_index": the index's dimension, "base": (kind,
    args...), "refine": bool}.  Prefixes OPQ{M}[_{d2}], PCA{d}, PCAR{d}, RR{d}; then Flat | IVF{n},Flat | IVF{n},PQ{M}[x8] | IVF{n},SQ8 |
    PQ{M}[x8] | SQ8; an optional trailing RFlat.  Anything else raises ValueError naming the token."""
    d = int(d)
    toks = [t.strip() for t in str(description).split(",")]
    if not toks or any(not t for t in toks):
        raise ValueError(f"index_factory: empty token in {description!r}")
    transforms, i, cur = [], 0, d
    while i < len(toks):
        t = toks[i]
        m = re.fullmatch(r"OPQ(\d+)(?:_(\d+))?", t)
        if m:
            M, d2 = int(m.group(1)), int(m.group(2)) if m.group(2) else cur
            if M <= 0 or d2 <= 0 or d2 % M or d2 > cur:
                raise ValueError(f"index_factory: token {t!r}: d2 = {d2} must be a positive multiple of M = {M} and at most {cur}")
            transforms.append(("OPQ", M, d2))
            cur = d2
        elif re.fullmatch(r"PCAR?(\d+)", t) or re.fullmatch(r"RR(\d+)", t):
            kind = "PCAR" if t.startswith("PCAR") else "PCA" if t.startswith("PCA") else "RR"
            dd = int(t[len(kind):])
            if dd <= 0 or (kind != "RR" and dd > cur):
                raise ValueError(f"index_factory: token {t!r}: the output dimension must be positive and at most {cur}")
            transforms.append((kind, dd))
            cur = dd
        else:
            break
        i += 1
    rest = toks[i:]
    refine = len(rest) > 1 and rest[-1] == "RFlat"
    if refine:
        rest = rest[:-1]
    if not rest:
        raise ValueError(f"index_factory: {description!r} names no index")

    def pq(tok):
        m = re.fullmatch(r"PQ(\d+)(?:x(\d+))?", tok)
        if not m:
            return None
        if m.group(2) and int(m.group(2)) != 8:
            raise ValueError(f"index_factory: token {tok!r}: only 8-bit product quantisers exist in this build")
        M = int(m.group(1))
        if M <= 0 or cur % M:
            raise ValueError(f"index_factory: token {tok!r}: the dimension {cur} is not a multiple of M = {M}")
        return M

    if rest[0] == "Flat":
        base, used = ("Flat",), 1
    elif re.fullmatch(r"IVF(\d+)", rest[0]):
        nlist = int(rest[0][3:])
        if nlist <= 0:
            raise ValueError(f"index_factory: token {rest[0]!r}: nlist must be positive")
        if len(rest) < 2:
            raise ValueError(f"index_factory: token {rest[0]!r} needs an encoding behind it (Flat, PQ{{M}}[x8] or SQ8)")
        if rest[1] == "Flat":
            base = ("IVFFlat", nlist)
        elif rest[1] == "SQ8":
            base = ("IVFSQ", nlist)
        elif pq(rest[1]) is not None:
            base = ("IVFPQ", nlist, pq(rest[1]))
        else:
            raise ValueError(f"index_factory: unknown token {rest[1]!r}")
        used = 2
    elif rest[0] == "SQ8":
        base, used = ("SQ",), 1
    elif pq(rest[0]) is not None:
        base, used = ("PQ", pq(rest[0])), 1
    else:
        raise ValueError(f"index_factory: unknown token {rest[0]!r}")
    if len(rest) > used:
        raise ValueError(f"index_factory: unexpected token {rest[used]!r}")
    if refine and base[0] == "IVFSQ":
        raise ValueError("index_factory: token 'RFlat': IndexRefineFlat over an IndexIVFScalarQuantizer is not supported in this build")
    if refine and base[0] == "SQ":
        raise ValueError("index_factory: token 'RFlat': IndexRefineFlat over an IndexScalarQuantizer is not supported in this build")
    if refine and transforms:
        raise ValueError("index_factory: token 'RFlat': IndexRefineFlat over an IndexPreTransform is not supported in this build")
    return {"transforms": transforms, "d_index": cur, "base": base, "refine": refine}


def index_factory(d, description, metric=_r.METRIC_L2, device=None):
    """faiss.index_factory(d, description, metric) over what this build has (parse_index_factory)."""
    spec = parse_index_factory(d, description)
    di, base = spec["d_index"], spec["base"]
    if base[0] == "Flat":
        ix = _r.IndexFlat(di, metric, device=device)
    elif base[0] == "PQ":
        ix = _r.IndexPQ(di, base[1], 8, metric, device=device)
    elif base[0] == "SQ":
        ix = _r.IndexScalarQuantizer(di, _r.ScalarQuantizer.QT_8bit, metric, device=device)
    elif base[0] == "IVFFlat":
        ix = _r.IndexIVFFlat(None, di, base[1], metric, device=device)
    elif base[0] == "IVFSQ":
        ix = _r.IndexIVFScalarQuantizer(None, di, base[1], _r.ScalarQuantizer.QT_8bit, metric, device=device)
    else:
        ix = _r.IndexIVFPQ(None, di, base[1], base[2], 8, metric, device=device)
    if spec["refine"]:
        ix = _r.IndexRefineFlat(ix)
    if spec["transforms"]:
        dev = ix._get("device")
        ix = IndexPreTransform(ix)
        cur = int(d)
        vts = []
        for t in spec["transforms"]:
            if t[0] == "OPQ":
                vts.append(OPQMatrix(cur, t[1], t[2], device=dev))
            elif t[0] == "RR":
                vts.append(RandomRotationMatrix(cur, t[1], device=dev))
            else:
                vts.append(PCAMatrix(cur, t[1], 0, t[0] == "PCAR", device=dev))
            cur = vts[-1].d_out
        for vt in reversed(vts):
            ix.prepend_transform(vt)
    return ix


def downcast_index(index):
    """faiss.downcast_index: a Python object here already is of its concrete class."""
    return index


def extract_index_ivf(index):
    """faiss.extract_index_ivf: the IVF index inside an IndexPreTransform / IndexRefineFlat (or the index itself); raises if there is none."""
    seen = index
    while True:
        if isinstance(seen, _r._IndexIVF):
            return seen
        if isinstance(seen, IndexPreTransform):
            seen = seen.index
        elif isinstance(seen, _r.IndexRefineFlat):
            seen = seen.base_index
        else:
            raise RuntimeError(f"extract_index_ivf: could not extract an IVF index from a {type(index).__name__}")
