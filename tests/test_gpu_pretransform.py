"""GPU: the vector transforms and IndexPreTransform.  rsx_vt_apply against tests/vt_ref.py bit for bit; a search through a
transform EQUAL to the search of the transformed data on every index kind; training through the chain; the PCA and OPQ numbers;
reconstruct, persistence, the factory and the refusals."""
import functools

import numpy as np
import pytest

import sq_ref
import vt_ref

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ------------------------------------------------------------------------------------------ apply
SHAPES = [(1, 8, 8), (130, 40, 24), (257, 100, 100), (129, 64, 160), (300, 768, 256), (200, 768, 768)]


@functools.lru_cache(maxsize=None)
def apply_case(n, d_in, d_out, f16, bias):
    """inputs and the reference's outputs, once per case: A a random rotation (so that the reverse form applies to every shape)"""
    rng = np.random.RandomState(n + d_in + d_out)
    A = vt_ref.random_rotation(d_in, d_out, 11)
    b = rng.randn(d_out).astype(F32) if bias else None
    x = rng.randn(n, d_in).astype(np.float16 if f16 else F32)
    y = vt_ref.apply(A, b, x)
    yin = (y * F32(1.0009765625)).astype(np.float16 if f16 else F32)      # the reverse form's own input: any values of the dtype
    return A, b, x, y, yin, vt_ref.reverse(A, b, yin)


def linear(gpu, A, b):
    lt = gpu.LinearTransform(A.shape[1], A.shape[0], b is not None)
    assert not lt.is_trained and lt.have_bias == (b is not None) and lt.b.shape == (0,)
    with pytest.raises(RuntimeError, match="not trained"):
        lt.apply(np.zeros((1, A.shape[1]), F32))
    lt.A = A
    if b is not None:
        lt.b = b
    lt.is_trained = True
    return lt


@pytest.mark.parametrize("form", ["numpy", "cuda"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("n,d_in,d_out", SHAPES)
def test_apply_and_reverse_bit_equal_to_reference(gpu, n, d_in, d_out, f16, bias, form):
    import torch
    A, b, x, y, yin, xback = apply_case(n, d_in, d_out, f16, bias)
    lt = linear(gpu, A, b)
    if form == "cuda":
        got = lt.apply(torch.from_numpy(x).cuda())
        assert got.is_cuda and got.dtype == torch.float32
        got = got.cpu().numpy()
    else:
        got = lt.apply(x)
        assert isinstance(got, np.ndarray) and got.dtype == F32
    assert got.shape == (n, d_out)
    assert np.array_equal(bits(got), bits(y)), f"apply differs at {np.argwhere(bits(got) != bits(y))[:3].tolist()}"
    assert np.array_equal(bits(lt.apply_py(x)), bits(y))
    # the reverse form: refused until the matrix is known to be orthonormal
    with pytest.raises(RuntimeError, match="non-orthonormal"):
        lt.reverse_transform(yin)
    if d_out <= d_in:
        assert lt.set_is_orthonormal() is True
    else:
        assert lt.set_is_orthonormal() is False      # FAISS's rule; the columns are orthonormal, which is what the transposed product needs
        lt.is_orthonormal = True
    back = lt.reverse_transform(torch.from_numpy(yin).cuda()).cpu().numpy() if form == "cuda" else lt.reverse_transform(yin)
    assert back.shape == (n, d_in)
    assert np.array_equal(bits(back), bits(xback)), f"reverse differs at {np.argwhere(bits(back) != bits(xback))[:3].tolist()}"


def test_apply_of_nothing_and_argument_checks(gpu):
    import torch
    A, b, x, y, _, _ = apply_case(130, 40, 24, False, True)
    lt = linear(gpu, A, b)
    e = lt.apply(np.zeros((0, 40), F32))
    assert isinstance(e, np.ndarray) and e.shape == (0, 24) and e.dtype == F32
    e = lt.apply(torch.zeros((0, 40), device="cuda"))
    assert e.is_cuda and tuple(e.shape) == (0, 24)
    with pytest.raises(AssertionError):
        lt.apply(np.zeros((3, 41), F32))
    # float64 input is read as float32 (as every entry point does); a new matrix replaces the old one
    assert np.array_equal(bits(lt.apply(x.astype(np.float64))), bits(y))
    lt.A = (2 * A).astype(F32)
    lt.b = np.zeros(24, F32)
    assert np.array_equal(bits(lt.apply(x)), bits(vt_ref.apply(2 * A, np.zeros(24, F32), x)))
    lt.A = A[:5]
    with pytest.raises(RuntimeError, match="shape"):
        lt.apply(x)
    rr = gpu.RandomRotationMatrix(40, 24)
    assert not rr.is_trained
    rr.train(x)
    assert rr.is_trained and rr.is_orthonormal and np.array_equal(rr.A, vt_ref.random_rotation(40, 24, 12345))
    rr.init(3)
    assert np.array_equal(rr.A, vt_ref.random_rotation(40, 24, 3))
    assert np.array_equal(bits(rr.apply(x)), bits(vt_ref.apply(rr.A, None, x)))


# ------------------------------------------------------------------------------------------ composition
KINDS = ["ivfpq", "pq", "ivfsq", "ivfflat", "flat"]
_tf, _pt = {}, {}


def transform(gpu, name):
    """the two transforms of the composition tests on set (B), with the reference's image of the set and of its queries"""
    if name not in _tf:
        c = sq_ref.inputs("B")
        if name == "rr":
            vt = gpu.RandomRotationMatrix(64, 64)
            vt.init(7)
        else:
            vt = gpu.OPQMatrix(64, 16)
            vt.niter = 3
            assert not vt.is_trained
            vt.train(c.x32)
            assert vt.is_trained and vt.is_orthonormal and len(vt.pq_errors) == 3
        _tf[name] = (vt, vt_ref.apply(vt.A, None, c.x32), vt_ref.apply(vt.A, None, c.q32))
    return _tf[name]


def new_base(gpu, kind, metric, c):
    if kind == "ivfpq":
        return gpu.IndexIVFPQ(None, c.d, c.nlist, 16, 8, metric)
    if kind == "pq":
        return gpu.IndexPQ(c.d, 16, 8, metric)
    if kind == "ivfsq":
        return gpu.IndexIVFScalarQuantizer(None, c.d, c.nlist, gpu.ScalarQuantizer.QT_8bit, metric)
    if kind == "ivfflat":
        return gpu.IndexIVFFlat(None, c.d, c.nlist, metric)
    return gpu.IndexFlat(c.d, metric)


def copy_trained(src, dst, kind):
    if kind in ("ivfpq", "ivfsq", "ivfflat"):
        dst.set_centroids(src.get_centroids())
    if kind in ("ivfpq", "pq"):
        dst.set_codebooks(src.get_codebooks())
    if kind == "ivfsq":
        dst.set_sq_trained(src.sq.trained)
    assert dst.is_trained


def pair(gpu, tf, kind, metric):
    """(IndexPreTransform over a base trained and filled through it, a second base with the first one's trained state filled with the
    reference's transformed set), once per case"""
    key = (tf, kind, metric)
    if key not in _pt:
        c = sq_ref.inputs("B")
        vt, xt, _ = transform(gpu, tf)
        base = new_base(gpu, kind, metric, c)
        pt = gpu.IndexPreTransform(vt, base)
        assert pt.d == 64 and pt.index is base and pt.chain == [vt] and pt.metric_type == metric and pt.ntotal == 0
        assert pt.is_trained == (kind == "flat")
        pt.train(c.x)
        assert pt.is_trained and base.is_trained
        if metric == 1:
            pt.add_chunk_rows = 2500          # three passes: order and ids are those of one add
        pt.add(c.x)
        assert pt.ntotal == c.n == base.ntotal
        base2 = new_base(gpu, kind, metric, c)
        copy_trained(base, base2, kind)
        base2.add(xt)
        for ix in (base, base2):
            if kind in ("ivfpq", "ivfsq", "ivfflat"):
                ix.nprobe = c.nprobe
        _pt[key] = (pt, base2)
    return _pt[key]


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tf", ["rr", "opq"])
def test_search_through_a_transform_equals_search_of_the_transformed_data(gpu, orc, tf, kind, metric):
    import torch
    c = sq_ref.inputs("B")
    vt, xt, qt = transform(gpu, tf)
    pt, base2 = pair(gpu, tf, kind, metric)
    base = pt.index
    if kind in ("flat", "ivfflat"):
        assert base.storage_dtype == "float32", "rotated vectors are not fp16-representable: the rows are stored widened"
    assert np.array_equal(base.list_sizes(), base2.list_sizes())
    for l in range(c.nlist if kind in ("ivfpq", "ivfsq", "ivfflat") else 1):
        (p1, i1), (p2, i2) = base.get_list(l), base2.get_list(l)
        assert np.array_equal(i1, i2), f"list {l}: ids"
        assert p1.dtype == p2.dtype and np.array_equal(p1.view(np.uint8), p2.view(np.uint8)), f"list {l}: codes / rows"
    for k in c.ks:
        D, I = pt.search(c.q, k)
        D2, I2 = base2.search(qt, k)
        assert isinstance(D, np.ndarray) and D.shape == (c.nq, k)
        assert np.array_equal(I, I2) and np.array_equal(bits(D), bits(D2)), f"k {k}"
        if kind == "ivfpq" and metric == 0:
            cen, cb = base.get_centroids(), base.get_codebooks()
            a, _ = orc.assign_ip(cen, xt)
            lm = orc.ListMajor(a, np.arange(c.n), orc.pq_encode(cb, orc.residuals(cen, xt, a)), c.nlist)
            Dr, Ir = orc.ivfpq_search(cen, cb, lm, qt, c.nprobe, k)
            assert np.array_equal(I, Ir) and np.array_equal(bits(D), bits(Dr)), f"k {k}: differs from the oracle over the transformed data"
    Dc, Ic = pt.search(torch.from_numpy(c.q).cuda(), 10)
    D2, I2 = base2.search(qt, 10)
    assert Dc.is_cuda and Ic.is_cuda
    assert np.array_equal(Ic.cpu().numpy(), I2) and np.array_equal(bits(Dc.cpu().numpy()), bits(D2))


@pytest.mark.parametrize("kind", KINDS)
def test_selectors_and_params_pass_through(gpu, kind):
    c = sq_ref.inputs("B")
    _, _, qt = transform(gpu, "rr")
    pt, base2 = pair(gpu, "rr", kind, 0)
    sel = gpu.IDSelectorRange(1000, 4000)
    ip = gpu.SearchParameters(sel=sel) if kind in ("flat", "pq") else gpu.SearchParametersIVF(sel=sel, nprobe=c.nprobe)
    params = gpu.SearchParametersPreTransform(index_params=ip)
    if kind in ("pq", "ivfsq"):      # the index's own refusal reaches the caller, and the handle answers as before
        with pytest.raises(RuntimeError, match="rsx error"):
            pt.search(c.q, 10, params=params)
    else:
        D, I = pt.search(c.q, 10, params)
        D2, I2 = base2.search(qt, 10, params=ip)
        assert ((I >= 1000) & (I < 4000)).all()
        assert np.array_equal(I, I2) and np.array_equal(bits(D), bits(D2))
    # a foreign params class is refused by the wrapper itself
    with pytest.raises(RuntimeError, match="IndexPreTransform"):
        pt.search(c.q, 10, params=ip)
    D, I = pt.search(c.q, 10, params=gpu.SearchParametersPreTransform())
    D2, I2 = base2.search(qt, 10)
    assert np.array_equal(I, I2) and np.array_equal(bits(D), bits(D2))


def test_range_search_and_removal_forward_to_the_index(gpu):
    c = sq_ref.inputs("B")
    vt, xt, qt = transform(gpu, "rr")
    pt = gpu.IndexPreTransform(vt, gpu.IndexFlat(64, 0))
    b2 = gpu.IndexFlat(64, 0)
    ids = np.arange(c.n, dtype=np.int64)[::-1].copy() + 10
    pt.add_with_ids(c.x[:3000], ids[:3000])
    b2.add_with_ids(xt[:3000], ids[:3000])
    D, _ = b2.search(qt[:8], 20)
    radius = float(D[:, -1].max())
    for got, want in zip(pt.range_search(c.q[:8], radius), b2.range_search(qt[:8], radius)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert pt.remove_ids(ids[:100]) == 100 == b2.remove_ids(ids[:100]) and pt.ntotal == 2900
    D, I = pt.search(c.q, 5)
    D2, I2 = b2.search(qt, 5)
    assert np.array_equal(I, I2) and np.array_equal(bits(D), bits(D2))
    with pytest.raises(RuntimeError, match="range_search"):      # the index's own refusal
        pair(gpu, "rr", "ivfpq", 0)[0].range_search(c.q[:2], 1.0)
    pt.reset()
    assert pt.ntotal == 0


# ------------------------------------------------------------------------------------------ training through the chain
def test_training_through_the_chain(gpu):
    c = sq_ref.inputs("B")
    pca = gpu.PCAMatrix(64, 32)
    base = gpu.IndexIVFPQ(None, 32, c.nlist, 8, 8, gpu.METRIC_INNER_PRODUCT)
    pt = gpu.IndexPreTransform(pca, base)
    assert pt.d == 64 and not pca.is_trained and not base.is_trained and not pt.is_trained
    with pytest.raises(RuntimeError, match="not trained"):
        pt.add(c.x)
    pt.train(c.x)
    assert pca.is_trained and base.is_trained and pt.is_trained and pca.is_orthonormal
    assert pca.A.shape == (32, 64) and pca.b.shape == (32,) and pca.mean.shape == (64,) and pca.PCAMat.shape == (64, 64)
    xt = vt_ref.apply(pca.A, pca.b, c.x32)
    direct = gpu.IndexIVFPQ(None, 32, c.nlist, 8, 8, gpu.METRIC_INNER_PRODUCT)
    direct.train(xt)
    assert np.array_equal(bits(base.get_centroids()), bits(direct.get_centroids())), "centroids differ from training on the transformed set"
    assert np.array_equal(bits(base.get_codebooks()), bits(direct.get_codebooks())), "codebooks differ from training on the transformed set"
    # a trained transform is left alone by a second train
    A0 = pca.A.copy()
    pt.train(c.x[:3000])
    assert np.array_equal(pca.A, A0)


# ------------------------------------------------------------------------------------------ PCA and OPQ numbers
@functools.lru_cache(maxsize=None)
def decaying():
    return (np.random.RandomState(1).randn(20000, 32) * 0.75 ** np.arange(32)).astype(F32)


def test_pca_numbers(gpu):
    x = decaying()
    A, b, mean, w, _ = vt_ref.pca_train(x, 8)
    gaps = (w[:8] - w[1:9]) / w[:8]
    assert gaps.min() >= 4e-3, "the test's own premise: separated eigenvalues"
    pca = gpu.PCAMatrix(32, 8)
    pca.train(x)
    rel = np.abs(pca.eigenvalues - w) / w
    dA = np.abs(pca.A.astype(np.float64) - A.astype(np.float64)).max()
    print(f"eigenvalues: max relative difference {rel.max():.3e}; A: max difference {dA:.3e} (2^-23 = {2.0 ** -23:.3e})")
    assert pca.eigenvalues.dtype == np.float64 and pca.eigenvalues.shape == (32,) and (np.diff(pca.eigenvalues) <= 0).all()
    assert rel.max() <= 1e-9
    assert dA <= 2.0 ** -23
    assert (pca.A[np.arange(8), np.abs(pca.A).argmax(1)] > 0).all(), "sign rule: the largest-magnitude component is positive"
    assert np.abs(pca.mean.astype(np.float64) - x.astype(np.float64).mean(0)).max() <= 2.0 ** -24
    want_b = (-(pca.A.astype(np.float64) @ pca.mean.astype(np.float64))).astype(F32)
    assert np.array_equal(bits(pca.b), bits(want_b))
    assert pca.is_orthonormal and pca.set_is_orthonormal()
    y = pca.apply(x[:500])
    assert np.array_equal(bits(y), bits(vt_ref.apply(pca.A, pca.b, x[:500])))
    assert np.array_equal(bits(pca.reverse_transform(y)), bits(vt_ref.reverse(pca.A, pca.b, y)))
    # whitening: rows scaled by eigenvalue ** -0.5 — unit variances, not orthonormal, no reverse
    wh = gpu.PCAMatrix(32, 8, -0.5)
    wh.train(x)
    assert not wh.is_orthonormal and not wh.set_is_orthonormal()
    Aw, bw, _, _, _ = vt_ref.pca_train(x, 8, -0.5)
    assert np.abs(wh.A.astype(np.float64) - Aw).max() <= 2.0 ** -22 * np.abs(Aw).max()
    yw = wh.apply(x)
    assert np.array_equal(bits(yw[:500]), bits(vt_ref.apply(wh.A, wh.b, x[:500])))
    assert np.abs(yw.astype(np.float64).var(0) - 1).max() <= 1e-3
    with pytest.raises(RuntimeError, match="non-orthonormal"):
        wh.reverse_transform(yw[:4])
    # PCAR: a rotation of the outputs in front; still orthonormal
    pr = gpu.PCAMatrix(32, 8, 0, True)
    pr.train(x)
    assert pr.set_is_orthonormal() and not np.array_equal(pr.A, pca.A)
    want = vt_ref.random_rotation(8, 8, 5).astype(np.float64)      # (the rotation itself is fp64 in the library: compare loosely)
    assert np.abs(pr.A.astype(np.float64) - want @ pca.A.astype(np.float64)).max() <= 2.0 ** -21


def pq_mse(gpu, x, M):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).cuda()
    ix = gpu.IndexPQ(x.shape[1], M, 8, gpu.METRIC_L2)
    ix.train(t)
    ix.add(t)
    return float(((t.double() - ix.reconstruct_batch(torch.arange(len(x), device="cuda")).double()) ** 2).sum(1).mean())


def test_opq_numbers(gpu):
    """The condition: the OPQ-rotated data quantises better than the randomly rotated and than the unrotated data, in the same run.  Reference on
    the CPU (vt_ref.pq_mse / random_rotation / opq_train): 0.3382 unrotated, 0.2230 randomly rotated, 0.0595 after eight OPQ iterations; the GPU
    printed the same four digits."""
    x = decaying()
    opq = gpu.OPQMatrix(32, 4)
    assert (opq.d_in, opq.d_out, opq.M, opq.niter, opq.max_train_points, opq.verbose) == (32, 32, 4, 50, 65536, False)
    opq.niter = 8
    opq.train(x)
    A = opq.A.astype(np.float64)
    dev = np.abs(A @ A.T - np.eye(32)).max()
    print(f"OPQ: max |A·Aᵀ - I| = {dev:.3e} (2^-22 = {2.0 ** -22:.3e}); quantisation error per iteration {[round(e, 4) for e in opq.pq_errors]}")
    assert dev <= 2.0 ** -22 and opq.is_orthonormal and opq.set_is_orthonormal()
    rr = gpu.RandomRotationMatrix(32, 32)
    rr.init(12345)
    plain, rand, best = pq_mse(gpu, x, 4), pq_mse(gpu, rr.apply(x), 4), pq_mse(gpu, opq.apply(x), 4)
    print(f"PQ mean squared reconstruction error, M = 4: unrotated {plain:.4f}, random rotation {rand:.4f}, OPQ (8 iterations) {best:.4f}")
    assert best < rand and best < plain
    sub = gpu.OPQMatrix(32, 4, 16)
    sub.niter = 2
    sub.train(x)
    As = sub.A.astype(np.float64)
    assert sub.A.shape == (16, 32) and np.abs(As @ As.T - np.eye(16)).max() <= 2.0 ** -22
    with pytest.raises(RuntimeError, match="d2"):
        gpu.OPQMatrix(32, 4, 64)


# ------------------------------------------------------------------------------------------ reconstruct, persistence, refusals
def test_reconstruct_family(gpu):
    import torch
    c = sq_ref.inputs("B")
    vt, _, _ = transform(gpu, "rr")
    pt, _ = pair(gpu, "rr", "ivfpq", 0)
    base = pt.index
    keys = np.array([5, 0, 5999, 17, 5], dtype=np.int64)
    want = vt_ref.reverse(vt.A, None, base.reconstruct_batch(keys))
    assert np.array_equal(bits(pt.reconstruct_batch(keys)), bits(want))
    assert np.array_equal(bits(pt.reconstruct(17)), bits(want[3])) and pt.reconstruct(17).shape == (64,)
    assert np.array_equal(bits(pt.reconstruct_n(10, 20)), bits(vt_ref.reverse(vt.A, None, base.reconstruct_n(10, 20))))
    got = pt.reconstruct_batch(torch.from_numpy(keys).cuda())
    assert got.is_cuda and np.array_equal(bits(got.cpu().numpy()), bits(want))
    D, I, R = pt.search_and_reconstruct(c.q, 10)
    Ds, Is = pt.search(c.q, 10)
    assert np.array_equal(I, Is) and np.array_equal(bits(D), bits(Ds)) and R.shape == (c.nq, 10, 64) and (I >= 0).all()
    assert np.array_equal(bits(R.reshape(-1, 64)), bits(pt.reconstruct_batch(I.reshape(-1))))
    # padding labels: every bit of the row set, as the index itself returns it
    small = gpu.IndexPreTransform(vt, gpu.IndexFlat(64, 1))
    small.add(c.x[:5])
    D, I, R = small.search_and_reconstruct(c.q[:3], 8)
    assert (I[:, 5:] == -1).all() and (R[:, 5:].view(np.uint32) == 0xFFFFFFFF).all()
    assert np.array_equal(bits(R[:, :5].reshape(-1, 64)), bits(small.reconstruct_batch(I[:, :5].reshape(-1))))
    # a chain with a transform that has no reverse
    wh = gpu.PCAMatrix(64, 32, -0.5)
    pw = gpu.IndexPreTransform(wh, gpu.IndexFlat(32, 1))
    pw.train(c.x)
    pw.add(c.x[:100])
    with pytest.raises(RuntimeError, match="non-orthonormal"):
        pw.reconstruct(3)


def test_write_and_read(gpu, tmp_path, monkeypatch):
    c = sq_ref.inputs("B")
    pca = gpu.PCAMatrix(64, 32)
    rr = gpu.RandomRotationMatrix(32, 32)
    base = gpu.IndexIVFPQ(None, 32, c.nlist, 8, 8, gpu.METRIC_L2)
    pt = gpu.IndexPreTransform(rr, base)
    pt.prepend_transform(pca)
    assert pt.chain == [pca, rr] and pt.d == 64
    pt.train(c.x)
    pt.add(c.x)
    base.nprobe = c.nprobe
    D, I = pt.search(c.q, 10)
    path = str(tmp_path / "pt.index")
    gpu.write_index(pt, path)
    assert open(path, "rb").read(4) == b"RSXT"
    back = gpu.read_index(path)
    assert isinstance(back, gpu.IndexPreTransform) and isinstance(back.index, gpu.IndexIVFPQ) and back.ntotal == c.n and back.d == 64
    assert [type(v) for v in back.chain] == [gpu.PCAMatrix, gpu.RandomRotationMatrix]
    for v, w in zip(back.chain, pt.chain):
        assert (v.d_in, v.d_out, v.have_bias, v.is_trained, v.is_orthonormal) == (w.d_in, w.d_out, w.have_bias, w.is_trained, w.is_orthonormal)
        assert np.array_equal(bits(v.A), bits(w.A)) and np.array_equal(bits(v.b), bits(w.b))
    p2 = back.chain[0]
    assert np.array_equal(bits(p2.mean), bits(pca.mean)) and np.array_equal(p2.eigenvalues, pca.eigenvalues) and np.array_equal(bits(p2.PCAMat), bits(pca.PCAMat))
    assert p2.eigen_power == 0 and p2.random_rotation is False
    back.index.nprobe = c.nprobe
    D2, I2 = back.search(c.q, 10)
    assert np.array_equal(I, I2) and np.array_equal(bits(D), bits(D2))
    # the FAISS format: refused both ways, the handle answers as before
    monkeypatch.setenv("RSX_INDEX_FORMAT", "faiss")
    with pytest.raises(RuntimeError, match="IndexPreTransform"):
        gpu.write_index(pt, str(tmp_path / "pt.faiss"))
    monkeypatch.delenv("RSX_INDEX_FORMAT")
    fake = tmp_path / "fake.faiss"
    fake.write_bytes(b"IxPT" + bytes(64))
    with pytest.raises(RuntimeError, match="IxPT"):
        gpu.read_index(str(fake))
    with pytest.raises(RuntimeError, match="several devices"):
        gpu.read_index(path, devices=[0, 0])
    D3, I3 = pt.search(c.q, 10)
    assert np.array_equal(I, I3) and np.array_equal(bits(D), bits(D3))


def test_refusals(gpu):
    c = sq_ref.inputs("B")
    _, _, qt = transform(gpu, "rr")
    pt, base2 = pair(gpu, "rr", "ivfflat", 0)
    with pytest.raises(RuntimeError, match="sharded"):
        gpu.IndexPreTransform(gpu.RandomRotationMatrix(64, 64), gpu.IndexIVFFlat(None, 64, 16, 0, devices=[0, 0]))
    with pytest.raises(RuntimeError, match="d_out"):
        gpu.IndexPreTransform(gpu.RandomRotationMatrix(64, 32), gpu.IndexFlat(64, 0))
    with pytest.raises(RuntimeError, match="d_out"):
        pt.prepend_transform(gpu.RandomRotationMatrix(32, 48))
    with pytest.raises(TypeError, match="VectorTransform"):
        gpu.IndexPreTransform(np.eye(64, dtype=F32), gpu.IndexFlat(64, 0))
    with pytest.raises(TypeError, match="IndexPreTransform"):
        gpu.IndexPreTransform(gpu.RandomRotationMatrix(64, 64), "Flat")
    with pytest.raises(RuntimeError, match="IndexPreTransform"):
        pt.search(c.q, 10, params=gpu.SearchParametersIVF(nprobe=2))
    with pytest.raises(AssertionError):
        pt.search(c.q[:, :60], 10)
    # IndexRefineFlat does not take an IndexPreTransform as its base in this build
    with pytest.raises(TypeError, match="IndexRefineFlat"):
        gpu.IndexRefineFlat(pt)
    assert len(pt.chain) == 1 and pt.d == 64
    D, I = pt.search(c.q, 10)
    D2, I2 = base2.search(qt, 10)
    assert np.array_equal(I, I2) and np.array_equal(bits(D), bits(D2))


# ------------------------------------------------------------------------------------------ factory, helpers
def test_factory_builds_what_the_hand_built_object_is(gpu):
    c = sq_ref.inputs("B")
    fx = gpu.index_factory(64, "OPQ16,IVF16,PQ16", gpu.METRIC_INNER_PRODUCT)
    assert isinstance(fx, gpu.IndexPreTransform) and isinstance(fx.chain[0], gpu.OPQMatrix) and isinstance(fx.index, gpu.IndexIVFPQ)
    assert (fx.chain[0].d_in, fx.chain[0].d_out, fx.chain[0].M, fx.index.nlist, fx.index.M, fx.metric_type) == (64, 64, 16, 16, 16, 0)
    hand = gpu.IndexPreTransform(gpu.OPQMatrix(64, 16), gpu.IndexIVFPQ(None, 64, 16, 16, 8, gpu.METRIC_INNER_PRODUCT))
    out = []
    for ix in (fx, hand):
        ix.chain[0].niter = 2
        assert not ix.is_trained
        ix.train(c.x)
        ix.add(c.x)
        gpu.extract_index_ivf(ix).nprobe = c.nprobe
        out.append(ix.search(c.q, 10))
    assert np.array_equal(bits(fx.chain[0].A), bits(hand.chain[0].A))
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(bits(out[0][0]), bits(out[1][0]))
    assert gpu.extract_index_ivf(fx) is fx.index and gpu.downcast_index(fx) is fx
    # the other forms construct what they name
    f2 = gpu.index_factory(64, "PCAR32,IVF16,SQ8")
    assert isinstance(f2.chain[0], gpu.PCAMatrix) and f2.chain[0].random_rotation and isinstance(f2.index, gpu.IndexIVFScalarQuantizer) and f2.index.d == 32
    assert f2.metric_type == gpu.METRIC_L2
    f3 = gpu.index_factory(64, "RR64,PQ16x8", gpu.METRIC_INNER_PRODUCT)
    assert isinstance(f3.chain[0], gpu.RandomRotationMatrix) and isinstance(f3.index, gpu.IndexPQ)
    f4 = gpu.index_factory(64, "IVF16,PQ16,RFlat")
    assert isinstance(f4, gpu.IndexRefineFlat) and gpu.extract_index_ivf(f4) is f4.base_index
    f5 = gpu.index_factory(64, "PCA32,RR32,Flat")
    assert [type(v) for v in f5.chain] == [gpu.PCAMatrix, gpu.RandomRotationMatrix] and isinstance(f5.index, gpu.IndexFlat) and f5.d == 64
    assert isinstance(gpu.index_factory(64, "IVF16,Flat", gpu.METRIC_INNER_PRODUCT), gpu.IndexIVFFlat)
    with pytest.raises(RuntimeError, match="extract"):
        gpu.extract_index_ivf(f5)
    with pytest.raises(ValueError, match="HNSW32"):
        gpu.index_factory(64, "HNSW32")
