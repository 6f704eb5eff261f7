"""Reference of the vector transforms: numpy and the unmodified CPU oracle.

apply / reverse are the canon of rsx_vt_apply — y_j = fp32(s_j + b_j) with s_j the sequential fp32 chain s = fmaf(x[t], A[j][t], s) —
taken from the oracle's own coarse quantiser: its score of query x against "centroid" A[j] IS that chain, and with nprobe = d_out it
returns every row.  The trainers restate rsx_vt.py's training in numpy fp64, with the oracle's product quantiser."""
import numpy as np

F32 = np.float32


def _orc():
    from oracle import oracle as orc
    orc.build()
    return orc


def apply(A, b, x):
    """A float32 [d_out, d_in], b float32 [d_out] or None, x [n, d_in] (fp16 widened exactly) -> float32 [n, d_out]."""
    A = np.ascontiguousarray(A, dtype=F32)
    x = np.ascontiguousarray(x).astype(F32)
    d_out = A.shape[0]
    if len(x) == 0:
        return np.zeros((0, d_out), dtype=F32)
    pid, ps = _orc().coarse_probe(A, x, d_out)
    assert (np.sort(pid, axis=1) == np.arange(d_out)).all(), "the oracle's probe did not return every row once"
    y = np.empty((len(x), d_out), dtype=F32)
    np.put_along_axis(y, pid, ps, axis=1)
    if b is not None and len(b):
        y = (y + np.asarray(b, dtype=F32)[None, :]).astype(F32)
    return y


def reverse(A, b, y):
    """x_t = chain over j of fmaf(fp32(y_j - b_j), A[j][t], s): the same chain through Aᵀ after the fp32 subtraction."""
    y = np.ascontiguousarray(y).astype(F32)
    if b is not None and len(b):
        y = (y - np.asarray(b, dtype=F32)[None, :]).astype(F32)
    return apply(np.ascontiguousarray(np.asarray(A, dtype=F32).T), None, y)


def random_rotation(d_in, d_out, seed):
    """float32 [d_out, d_in]: QR (fp64, R's diagonal made positive) of a RandomState(seed) normal matrix, rounded once."""
    lo, hi = min(d_in, d_out), max(d_in, d_out)
    g = np.random.RandomState(seed).randn(hi, lo)
    q, r = np.linalg.qr(g)
    q = q * np.where(np.diag(r) < 0, -1.0, 1.0)[None, :]
    return (q.T if d_out <= d_in else q).astype(F32)


def pca_train(x, d_out, eigen_power=0.0):
    """-> (A float32 [d_out, d_in], b float32 [d_out], mean float32, eigenvalues float64 descending, rows float64 = signed eigenvectors)."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=0)
    c = x - mean
    cov = c.T @ c / len(x)
    w, v = np.linalg.eigh(cov)
    order = np.argsort(-w, kind="stable")
    w, v = w[order], v[:, order].T
    big = np.abs(v).argmax(axis=1)
    v = v * np.where(v[np.arange(len(v)), big] < 0, -1.0, 1.0)[:, None]
    A = v.astype(F32)[:d_out].astype(np.float64)      # (the library keeps the eigenvectors as float32: PCAMat)
    if eigen_power:
        A = A * (w[:d_out] ** eigen_power)[:, None]
    A = A.astype(F32)
    mean32 = mean.astype(F32)
    b = (-(A.astype(np.float64) @ mean32.astype(np.float64))).astype(F32)
    return A, b, mean32, w, v


def pq_train_decode(x, M, niter_pq=25, seed=1234):
    """Train the oracle's product quantiser on x (the library's subsample and seed) and return the decoded x."""
    orc = _orc()
    x = np.ascontiguousarray(x, dtype=F32)
    cb = orc.pq_train(x[orc.kmeans_sample(len(x), 256, 256, seed)], M, niter_pq, seed)
    codes = orc.pq_encode(cb, x)
    return np.concatenate([cb[m][codes[:, m]] for m in range(M)], axis=1)


def pq_mse(x, M):
    """mean squared reconstruction error of a product quantiser trained on x"""
    x = np.ascontiguousarray(x, dtype=F32)
    return float(((x.astype(np.float64) - pq_train_decode(x, M)) ** 2).sum(1).mean())


def opq_train(x, M, d2, niter, seed=1234):
    """-> A float32 [d2, d]: alternating minimisation from random_rotation(d, d2, seed)."""
    x = np.ascontiguousarray(x, dtype=F32)
    A = random_rotation(x.shape[1], d2, seed)
    for _ in range(niter):
        xr = apply(A, None, x)
        xhat = pq_train_decode(xr, M)
        u, _, vt = np.linalg.svd(x.astype(np.float64).T @ xhat.astype(np.float64), full_matrices=False)
        A = (u @ vt).T.astype(F32)
    return A
