"""GPU: IndexRefineFlat / rsx_refine (FAISS IndexRefineFlat: search the base for k * k_factor candidates, re-score exactly those
against the stored rows, keep k) against the CPU oracle.

Every expected result is the ORACLE's composition, never the code under test's: the candidate labels are the base's oracle search at
k_base (orc.ivfpq_search / orc.ivfflat_search / test_gpu_pq.oracle_search), then per query orc.flat_search(q[i], x[cands], k, metric,
ids=cands) over the non-negative labels, padded with -1 / -+inf.  assert_same_results = ids and fp32 scores bit-equal.  The inputs are
the project's fp16 synth vectors and queries: fp64 sums of their products do not depend on the order of the terms."""
import ctypes
import os
import pickle

import numpy as np
import pytest

from util import assert_same_results

pytestmark = pytest.mark.gpu

NQ = 1024


class Kit:
    """One base kind: data, the trained parameters, the oracle's view of the lists and the populated IndexRefineFlat."""


_KITS = {}

BASES = {
    #  name         kind       d    M   layout nlist n      metric
    "ivfpq768": ("IVFPQ", 768, 96, 2, 64, 20011, 0),
    "ivfpq64l2": ("IVFPQ", 64, 16, 1, 32, 50021, 1),
    "pq64": ("PQ", 64, 16, None, 1, 20000, 0),
    "ivfflat100": ("IVFFlat", 100, 0, None, 16, 5000, 0),      # row padding: ld = 128
}


def kit(gpu, orc, name):
    if name in _KITS:
        return _KITS[name]
    kind, d, M, layout, nlist, n, metric = BASES[name]
    t = Kit()
    t.kind, t.d, t.nlist, t.n, t.metric = kind, d, nlist, n, metric
    t.x = orc.synth_vectors(d, 64, 1234, 10000, 0.5, 0, n)
    t.q = orc.synth_queries(d, 64, 1234, 10000, 0.5, n, 999, 0.1, 0, NQ)
    t.x32, t.q32 = t.x.astype(np.float32), t.q.astype(np.float32)
    ids = np.arange(n)
    if kind == "PQ":
        import test_gpu_pq
        t.cb = test_gpu_pq.codebooks_for(gpu, orc, d, M)
        t.codes = orc.pq_encode(t.cb, t.x32)
        base = gpu.IndexPQ(d, M, 8, metric)
        base.set_codebooks(t.cb)
        t.base_search = lambda q32, kb, nprobe, keep=None: test_gpu_pq.oracle_search(orc, t.cb, t.codes, q32, kb, metric)[1]
    else:
        t.cen = orc.kmeans(0, t.x32, nlist, 4, 1234)
        t.a, _ = orc.assign_ip(t.cen, t.x32)
        if kind == "IVFPQ":
            res = orc.residuals(t.cen, t.x32, t.a)
            t.cb = orc.pq_train(res[:4000], M, 3, 1234)
            t.codes = orc.pq_encode(t.cb, res)
            base = gpu.IndexIVFPQ(gpu.IndexFlatIP(d), d, nlist, M, 8, metric)
            if base._get("pq_layout") != layout:
                base.set_param("pq_layout", layout)
            assert base._get("pq_layout") == layout
            base.set_centroids(t.cen); base.set_codebooks(t.cb)

            def base_search(q32, kb, nprobe, keep=None):
                m = np.ones(n, bool) if keep is None else keep
                lm = orc.ListMajor(t.a[m], ids[m], t.codes[m], nlist)
                return orc.ivfpq_search(t.cen, t.cb, lm, q32, nprobe, kb, metric=metric)[1]
        else:
            base = gpu.IndexIVFFlat(gpu.IndexFlatIP(d), d, nlist, metric)
            base.set_centroids(t.cen)

            def base_search(q32, kb, nprobe, keep=None):
                m = np.ones(n, bool) if keep is None else keep
                lm = orc.ListMajor(t.a[m], ids[m], t.x32[m], nlist)
                return orc.ivfflat_search(metric, t.cen, lm, q32, nprobe, kb)[1]
        t.base_search = base_search
    t.index = gpu.IndexRefineFlat(base)
    t.index.add(t.x)
    assert t.index.ntotal == t.index.base_index.ntotal == t.index.refine_index.ntotal == n
    assert t.index.refine_index.storage_dtype == "float16"
    _KITS[name] = t
    return t


def refine_expected(orc, x32, q32, labels, k, metric):
    """The oracle's exact re-order of the oracle's candidates."""
    nq = len(q32)
    D = np.full((nq, k), -np.inf if metric == 0 else np.inf, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        c = labels[i][labels[i] >= 0]
        if len(c):
            kk = min(k, len(c))
            D[i, :kk], I[i, :kk] = orc.flat_search(q32[i:i + 1], x32[c], kk, metric, ids=c)
    return D, I


def set_nprobe(t, nprobe):
    if t.kind != "PQ":
        t.index.base_index.nprobe = nprobe


# ------------------------------------------------------------------------------------------ 1. parity across base kinds
CASES = [(1, 1, 64, 4), (10, 10, 1024, 4), (100, 1.5, 64, 4), (10, 409.6, 7, 4), (1000, 4.096, 1, 1)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "k%d-f%s-nq%d-np%d" % c)
@pytest.mark.parametrize("name", list(BASES))
def test_parity_with_the_oracle_composition(gpu, orc, name, case):
    k, k_factor, nq, nprobe = case
    t = kit(gpu, orc, name)
    k_base = int(k * k_factor)
    assert k_base == {(1, 1): 1, (10, 10): 100, (100, 1.5): 150, (10, 409.6): 4096, (1000, 4.096): 4096}[(k, k_factor)]
    set_nprobe(t, nprobe)
    t.index.k_factor = k_factor
    q, q32 = t.q[:nq], t.q32[:nq]
    labels = t.base_search(q32, k_base, nprobe)
    assert np.array_equal(t.index.base_index.search(q, k_base)[1], labels), "the GPU base's labels differ from the oracle's"
    if (k, nprobe) == (1000, 1) and t.kind != "PQ":
        assert (labels < 0).any(), "one probed list: candidate slots are padding"
    Dr, Ir = refine_expected(orc, t.x32, q32, labels, k, t.metric)
    D, I = t.index.search(q, k)
    assert isinstance(D, np.ndarray) and D.dtype == np.float32 and I.dtype == np.int64
    assert_same_results(D, I, Dr, Ir, f"{name} k={k} k_factor={k_factor} nq={nq} nprobe={nprobe}")
    t.index.k_factor = 1.0


@pytest.mark.parametrize("name", list(BASES))
def test_query_forms_and_search_parameters(gpu, orc, name):
    import torch
    t = kit(gpu, orc, name)
    k, k_factor, nq, nprobe = 10, 10, 64, 4
    set_nprobe(t, nprobe)
    q, q32 = t.q[:nq], t.q32[:nq]
    Dr, Ir = refine_expected(orc, t.x32, q32, t.base_search(q32, 100, nprobe), k, t.metric)
    t.index.k_factor = k_factor
    want = t.index.search(q, k)
    assert_same_results(*want, Dr, Ir, f"{name}: fp16 numpy queries")
    assert_same_results(*t.index.search(q32, k), Dr, Ir, f"{name}: fp32 numpy queries")
    for arr in (q, q32):                                   # CUDA tensors in -> CUDA tensors out
        D, I = t.index.search(torch.from_numpy(arr).cuda(), k)
        assert D.is_cuda and I.is_cuda and D.dtype == torch.float32 and I.dtype == torch.int64
        assert_same_results(D.cpu().numpy(), I.cpu().numpy(), Dr, Ir, f"{name}: CUDA {arr.dtype} queries")
    # the per-call k_factor equals the attribute
    t.index.k_factor = 1.0
    got = t.index.search(q, k, params=gpu.IndexRefineSearchParameters(k_factor=k_factor))
    assert_same_results(*got, Dr, Ir, f"{name}: IndexRefineSearchParameters(k_factor)")
    assert t.index.k_factor == 1.0
    with pytest.raises(RuntimeError, match="incorrect type"):
        t.index.search(q, k, params=gpu.SearchParameters())
    with pytest.raises(AssertionError, match="k_factor"):
        t.index.search(q, k, params=gpu.IndexRefineSearchParameters(k_factor=0.5))
    with pytest.raises(RuntimeError, match="rsx error -6"):            # k_base > 4096: the base's own refusal
        t.index.search(q[:2], 10, params=gpu.IndexRefineSearchParameters(k_factor=500))
    assert_same_results(*t.index.search(q, k, params=gpu.IndexRefineSearchParameters(k_factor=k_factor)), Dr, Ir, f"{name}: after the refusals")
    if t.kind == "PQ":
        return
    # a selector and a per-call nprobe travel to the base unchanged: the same composition over the filtered oracle candidates
    lo, hi = t.n // 5, t.n // 5 * 3
    keep = (np.arange(t.n) >= lo) & (np.arange(t.n) < hi)
    set_nprobe(t, 1)
    for np_call in (2, 5):
        labels = t.base_search(q32, 100, np_call, keep)
        assert ((labels < 0) | ((labels >= lo) & (labels < hi))).all()
        Df, If = refine_expected(orc, t.x32, q32, labels, k, t.metric)
        inner = gpu.SearchParametersIVF(nprobe=np_call, sel=gpu.IDSelectorRange(lo, hi))
        got = t.index.search(q, k, params=gpu.IndexRefineSearchParameters(k_factor=k_factor, base_index_params=inner))
        assert_same_results(*got, Df, If, f"{name}: selector [{lo}, {hi}) and nprobe {np_call} through base_index_params")
    assert t.index.base_index.nprobe == 1


# ------------------------------------------------------------------------------------------ 2. widened storage
def test_widened_refine_store(gpu, orc):
    t = kit(gpu, orc, "ivfflat100")
    x32 = t.x32.copy()
    x32[777, 3] = 1.0 + 2.0 ** -12          # not an fp16 value; products with fp16 queries still sum exactly in fp64
    assert np.float32(np.float16(x32[777, 3])) != x32[777, 3]
    base = gpu.IndexIVFFlat(gpu.IndexFlatIP(t.d), t.d, t.nlist, t.metric)
    base.set_centroids(t.cen)
    ix = gpu.IndexRefineFlat(base)
    ix.add(t.x[:700])
    assert ix.refine_index.storage_dtype == "float16"
    ix.add(x32[700:])
    assert ix.refine_index.storage_dtype == "float32" and ix.ntotal == t.n
    a, _ = orc.assign_ip(t.cen, x32)
    lm = orc.ListMajor(a, np.arange(t.n), x32, t.nlist)
    base.nprobe = 4
    qs = np.concatenate([t.q32[:63], x32[777:778].astype(np.float16).astype(np.float32)], 0)      # the last query sits on the widened row
    for k, k_factor in ((10, 10), (100, 1.5), (1, 1)):
        ix.k_factor = k_factor
        labels = orc.ivfflat_search(t.metric, t.cen, lm, qs, 4, int(k * k_factor))[1]
        assert np.array_equal(base.search(qs, int(k * k_factor))[1], labels)
        Dr, Ir = refine_expected(orc, x32, qs, labels, k, t.metric)
        assert_same_results(*ix.search(qs, k), Dr, Ir, f"widened rows k={k} k_factor={k_factor}")
    assert 777 in ix.search(qs, 10)[1][63]


# ------------------------------------------------------------------------------------------ 3. the raw entry point
def raw_refine(gpu, flat, q, labels, k, kc=None, device_labels=False, expect=0):
    import torch
    q = np.ascontiguousarray(q)
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    nq = q.shape[0]
    kc = labels.shape[1] if kc is None else kc
    D = np.full((nq, max(k, 1)), 123.0, np.float32)
    I = np.full((nq, max(k, 1)), -7, np.int64)
    dl = torch.from_numpy(labels).cuda() if device_labels else None
    lp = ctypes.c_void_p(dl.data_ptr()) if device_labels else labels.ctypes.data_as(ctypes.c_void_p)
    if device_labels:
        torch.cuda.synchronize()
    st = gpu.lib().rsx_refine(flat._h, ctypes.c_int64(nq), q.ctypes.data_as(ctypes.c_void_p), 1 if q.dtype == np.float16 else 0, int(kc), lp,
                              int(k), D.ctypes.data_as(ctypes.c_void_p), I.ctypes.data_as(ctypes.c_void_p))
    assert st == expect, f"rsx_refine returned {st} ({gpu.lib().rsx_last_error().decode()}), expected {expect}"
    return D, I


@pytest.mark.parametrize("metric", [0, 1], ids=["ip", "l2"])
def test_raw_entry_point(gpu, orc, metric):
    d, n, nq = 100, 3000, 5
    x = orc.synth_vectors(d, 8, 1234, 10000, 0.5, 0, n)
    x[41] = x[40]; x[42] = x[40]                           # equal rows: equal scores, ordered by label
    q = orc.synth_queries(d, 8, 1234, 10000, 0.5, n, 999, 0.1, 0, nq)
    x32, q32 = x.astype(np.float32), q.astype(np.float32)
    flat = gpu.IndexFlat(d, metric)
    flat.add(x)
    rng = np.random.RandomState(3)

    def check(labels, k, what, **kw):
        labels = np.asarray(labels, dtype=np.int64)
        Dr, Ir = refine_expected(orc, x32, q32[:len(labels)], labels, k, metric)
        for dev in (False, True):                          # host labels and device labels
            D, I = raw_refine(gpu, flat, q[:len(labels)], labels, k, device_labels=dev, **kw)
            assert_same_results(D, I, Dr, Ir, f"{what} ({'device' if dev else 'host'} labels)")
        return Dr, Ir

    # duplicates (each scored, both emitted, adjacent), equal rows under different labels, -1 in the middle of a row
    row = [7, 42, -1, 7, 40, 2999, -1, 41, 0, 7, 13]
    labels = np.array([row, row[::-1], [5] * 11, [-1] * 11, list(range(100, 111))])
    D, I = check(labels, 11, "duplicates and padding, k = kc")
    for r in (0, 1):
        pos = np.nonzero(I[r] == 7)[0]
        assert len(pos) == 3 and pos[2] - pos[0] == 2, "the three copies of label 7 sit next to each other"
        eq = [int(np.nonzero(I[r] == v)[0][0]) for v in (40, 41, 42)]
        assert eq[1] == eq[0] + 1 and eq[2] == eq[0] + 2 and D[r, eq[0]] == D[r, eq[2]], "equal scores are ordered by label"
        assert (I[r, 9:] == -1).all() and np.isinf(D[r, 9:]).all()
    assert (I[2] == 5).all() and (D[2] == D[2, 0]).all()
    assert (I[3] == -1).all() and (D[3] == (-np.inf if metric == 0 else np.inf)).all()      # all -1
    check(labels, 3, "k < kc")
    check(labels[:, :1], 1, "kc = 1")
    check(np.full((nq, 1), -1), 1, "kc = 1, all -1")
    # past the rank sort (kc > 512): the bitonic network, kc not a power of two, duplicates and padding mixed in
    big = rng.randint(-1, n, size=(nq, 777))
    big[:, 100:140] = big[:, 300:340]
    check(big, 777, "kc = 777, k = kc")
    check(big, 10, "kc = 777, k = 10")
    check(rng.randint(0, n, size=(2, 4096)), 4096, "kc = k = 4096")
    check(rng.randint(0, n, size=(nq, 512)), 512, "kc = 512: the largest rank sort")
    check(rng.randint(0, n, size=(nq, 513)), 20, "kc = 513: the smallest network")

    # every refusal leaves the handle usable
    good = labels[:, :4]
    Dg, Ig = refine_expected(orc, x32, q32, good, 2, metric)

    def still_right(what):
        assert_same_results(*raw_refine(gpu, flat, q, good, 2), Dg, Ig, f"a correct call after the refusal: {what}")

    ivf = gpu.IndexIVFFlat(None, d, 4, metric)
    raw_refine(gpu, ivf, q, good, 2, expect=-1)                                   # not a Flat handle
    pq = gpu.IndexPQ(d, 10, 8, metric)
    raw_refine(gpu, pq, q, good, 2, expect=-1)
    with_ids = gpu.IndexFlat(d, metric)
    with_ids.add_with_ids(x[:100], np.arange(100, dtype=np.int64) + 1000)
    raw_refine(gpu, with_ids, q, good, 2, expect=-6)                              # labels are positions
    assert "explicit ids" in gpu.lib().rsx_last_error().decode()
    sharded = gpu.IndexFlat(d, metric, devices=[0, 0])
    sharded.add(x[:100])
    raw_refine(gpu, sharded, q, good, 2, expect=-6)
    raw_refine(gpu, flat, q, np.zeros((nq, 4097), np.int64), 10, expect=-6); still_right("kc > 4096")
    raw_refine(gpu, flat, q, good, 5, expect=-1); still_right("k > kc")
    raw_refine(gpu, flat, q, good, 0, expect=-1); still_right("k < 1")
    bad = good.copy(); bad[3, 2] = n                                               # one label equal to ntotal
    for dev in (False, True):
        raw_refine(gpu, flat, q, bad, 2, device_labels=dev, expect=-1)
        assert "ntotal" in gpu.lib().rsx_last_error().decode()
        still_right("a label equal to ntotal")
    bad[3, 2] = 2 ** 40
    raw_refine(gpu, flat, q, bad, 2, expect=-1); still_right("a label far past ntotal")
    assert flat.get_timing("refine_calls") > 0 and flat.get_timing("refine_candidates") > 0
    flat.set_param("profile", 1)
    raw_refine(gpu, flat, q, good, 2)
    assert flat.get_timing("refine_calls") == 1 and flat.get_timing("refine_candidates") == nq * 4 and flat.get_timing("refine_ms") > 0


# ------------------------------------------------------------------------------------------ 4. ordering property
def test_refining_never_loses_a_true_neighbour(gpu, orc):
    """Every true neighbour among the base's candidates survives the exact re-order, so per query
    |refined & truth@10| >= |base top-10 & truth@10|; the three mean recalls are printed."""
    t = kit(gpu, orc, "ivfpq64l2")
    nq, k = 256, 10
    set_nprobe(t, t.nlist)
    q = t.q[:nq]
    truth = orc.flat_search(t.q32[:nq], t.x32, k, t.metric)[1]
    base10 = t.index.base_index.search(q, k)[1]
    hits = lambda I: np.array([len(set(I[i]) & set(truth[i])) for i in range(nq)])
    hb = hits(base10)
    print(f"\nrecall@10 of the base alone: {hb.mean() / k:.4f}")
    last = hb
    for k_factor in (1, 4, 10):
        t.index.k_factor = k_factor
        hr = hits(t.index.search(q, k)[1])
        print(f"recall@10 refined, k_factor {k_factor}: {hr.mean() / k:.4f}")
        assert (hr >= hb).all(), f"k_factor {k_factor}: a refined result holds fewer true neighbours than the base's top {k}"
        assert (hr >= last).all(), "more candidates never lose a true neighbour"
        last = hr
    t.index.k_factor = 1.0


# ------------------------------------------------------------------------------------------ 5. class behaviour
def test_class_behaviour(gpu, orc, tmp_path, monkeypatch):
    t = kit(gpu, orc, "ivfpq64l2")
    d, nlist, M = t.d, t.nlist, 16
    base = gpu.IndexIVFPQ(gpu.IndexFlatIP(d), d, nlist, M, 8, t.metric)
    ix = gpu.IndexRefineFlat(base)
    assert ix.base_index is base and isinstance(ix.refine_index, gpu.IndexFlat)
    assert (ix.d, ix.metric_type, ix.ntotal, ix.is_trained, ix.k_factor) == (d, t.metric, 0, False, 1.0)
    assert ix.refine_index.metric_type == t.metric and ix.refine_index._get("device") == base._get("device")
    ix.train(t.x[:8000])
    assert ix.is_trained and base.is_trained
    x = t.x[:6000]
    ix.add(x[:2500])
    assert ix.ntotal == base.ntotal == ix.refine_index.ntotal == 2500
    ix.add(x[2500:])
    assert ix.ntotal == base.ntotal == ix.refine_index.ntotal == 6000
    ix.reset()
    assert ix.ntotal == base.ntotal == ix.refine_index.ntotal == 0
    ix.add(x)
    assert ix.ntotal == base.ntotal == ix.refine_index.ntotal == 6000
    with pytest.raises(RuntimeError, match="add_with_ids not implemented"):
        ix.add_with_ids(x[:3], np.arange(3))
    with pytest.raises(RuntimeError, match="remove_ids not implemented"):
        ix.remove_ids(np.arange(3))
    assert ix.ntotal == 6000
    # bases that cannot be refined
    with_ids = gpu.IndexFlat(d, t.metric)
    with_ids.add_with_ids(x[:10], np.arange(10) + 5)
    with pytest.raises(RuntimeError, match="explicit ids"):
        gpu.IndexRefineFlat(with_ids)
    ivf_ids = gpu.IndexIVFFlat(None, d, nlist, t.metric)
    ivf_ids.set_centroids(base.get_centroids())
    late = gpu.IndexRefineFlat(ivf_ids)
    ivf_ids.add_with_ids(x[:10], np.arange(10) + 5)        # explicit ids arriving behind the wrapper's back: refused on add
    with pytest.raises(RuntimeError, match="explicit ids"):
        late.add(x[:10])
    with pytest.raises(RuntimeError, match="sharded"):
        gpu.IndexRefineFlat(gpu.IndexIVFPQ(None, d, nlist, M, 8, t.metric, devices=[0, 0]))
    with pytest.raises(TypeError):
        gpu.IndexRefineFlat(ix)
    # a Flat base: the refined result is the exact search itself
    fb = gpu.IndexRefineFlat(gpu.IndexFlat(d, t.metric))
    fb.k_factor = 3
    fb.add(x)
    assert_same_results(*fb.search(t.q[:20], 10), *orc.flat_search(t.q32[:20], x.astype(np.float32), 10, t.metric), "Flat base")
    # the oracle composition on this index (GPU-trained parameters, exported as the oracle needs them)
    cen, cb = base.get_centroids(), base.get_codebooks()
    x32 = x.astype(np.float32)
    a, _ = orc.assign_ip(cen, x32)
    lm = orc.ListMajor(a, np.arange(len(x)), orc.pq_encode(cb, orc.residuals(cen, x32, a)), nlist)
    base.nprobe = 6
    ix.k_factor = 7.5
    q, q32 = t.q[:50], t.q32[:50]
    labels = orc.ivfpq_search(cen, cb, lm, q32, 6, 75, metric=t.metric)[1]
    Dr, Ir = refine_expected(orc, x32, q32, labels, 10, t.metric)
    assert_same_results(*ix.search(q, 10), Dr, Ir, "trained and populated through the class")
    # save / load in both formats
    for fmt, magic in (("", b"RSXR"), ("faiss", b"IxRF")):
        monkeypatch.setenv("RSX_INDEX_FORMAT", fmt)
        path = str(tmp_path / f"refine_{fmt or 'rsx'}.index")
        gpu.write_index(ix, path)
        assert open(path, "rb").read(4) == magic
        if not fmt:
            assert sorted(os.listdir(tmp_path)) == ["refine_rsx.index", "refine_rsx.index.base", "refine_rsx.index.refine"]
            assert open(path + ".base", "rb").read(4) == b"RSX1" and open(path + ".refine", "rb").read(4) == b"RSX1"
        jx = gpu.read_index(path)
        assert isinstance(jx, gpu.IndexRefineFlat) and jx.k_factor == 7.5
        if not fmt:                                        # the manifest keeps the attribute exactly (IxRF: FAISS's float32)
            ix.k_factor = 4.096
            gpu.write_index(ix, path)
            assert gpu.read_index(path).k_factor == 4.096
            ix.k_factor = 7.5
        assert jx.ntotal == jx.base_index.ntotal == jx.refine_index.ntotal == 6000 and jx.metric_type == t.metric
        assert isinstance(jx.base_index, gpu.IndexIVFPQ) and jx.base_index.nprobe == 6
        assert_same_results(*jx.search(q, 10), Dr, Ir, f"after a {magic.decode()} round trip")
        with pytest.raises(RuntimeError, match="several devices"):
            gpu.read_index(path, devices=[0, 0])
    monkeypatch.setenv("RSX_INDEX_FORMAT", "")


# ------------------------------------------------------------------------------------------ 6. config key
class NS(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def test_config_key_through_the_indexer(gpu, orc, tmp_path):
    """cfg.datastore.index.refine_k_factor: a 5 000-vector IVF-PQ datastore built, searched, saved and re-loaded through the mirror's
    Indexer equals the class used directly on the same trained parameters."""
    from src.indicies.base import Indexer
    d, per, k, nlist, M = 64, 2500, 5, 8, 16
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "emb")); os.makedirs(os.path.join(root, "psg"))
    embs = []
    for s in range(2):
        e = orc.synth_vectors(d, 16, 11, 100 + s, 0.5, 0, per)
        embs.append(e)
        with open(os.path.join(root, "emb", f"passages_{s:02d}.pkl"), "wb") as f:
            pickle.dump((list(range(per)), e), f)
        with open(os.path.join(root, "psg", f"raw_passages-{s}-of-2.pkl"), "wb") as f:
            pickle.dump([{"text": f"s{s}c{c}"} for c in range(per)], f)
    x = np.concatenate(embs, 0)
    q = orc.synth_queries(d, 16, 11, 100, 0.5, per, 7, 0.1, 0, 40)

    def cfg(**extra):
        idx = NS(index_type="IVFPQ", index_shard_ids=[0, 1], projection_size=d, sample_train_size=4000, ncentroids=nlist, probe=3,
                 n_subquantizers=M, n_bits=8, **extra)
        return NS(datastore=NS(embedding=NS(embedding_dir=os.path.join(root, "emb"), prefix="passages",
                                            passages_dir=os.path.join(root, "psg")), index=idx))
    np.random.seed(5)
    built = Indexer(cfg(refine_k_factor=6))
    ix = built.datastore.index
    assert isinstance(ix, gpu.IndexRefineFlat) and ix.k_factor == 6.0 and ix.base_index.nprobe == 3
    assert ix.ntotal == ix.refine_index.ntotal == 2 * per
    # the class used directly, on the parameters the facade trained
    base = gpu.IndexIVFPQ(gpu.IndexFlatIP(d), d, nlist, M, 8, gpu.METRIC_INNER_PRODUCT)
    base.set_centroids(ix.base_index.get_centroids()); base.set_codebooks(ix.base_index.get_codebooks())
    direct = gpu.IndexRefineFlat(base)
    direct.k_factor = 6
    direct.add(x)
    base.nprobe = 3
    Dd, Id = direct.search(q, k)
    assert_same_results(*ix.search(q, k), Dd, Id, "the facade's index against the class used directly")
    # ... which is the oracle's composition
    cen, cb = base.get_centroids(), base.get_codebooks()
    x32, q32 = x.astype(np.float32), q.astype(np.float32)
    a, _ = orc.assign_ip(cen, x32)
    lm = orc.ListMajor(a, np.arange(len(x)), orc.pq_encode(cb, orc.residuals(cen, x32, a)), nlist)
    Dr, Ir = refine_expected(orc, x32, q32, orc.ivfpq_search(cen, cb, lm, q32, 3, 30)[1], k, 0)
    assert_same_results(Dd, Id, Dr, Ir, "the class against the oracle composition")
    scores, passages, db_ids = built.search(q, k)
    assert np.array_equal(np.asarray(scores, dtype=np.float32), Dd)
    again = Indexer(cfg(refine_k_factor=6))                # load path: the RSXR manifest under the reference's file name
    jx = again.datastore.index
    assert isinstance(jx, gpu.IndexRefineFlat) and jx.k_factor == 6.0 and jx.base_index.nprobe == 3
    assert_same_results(*jx.search(q, k), Dd, Id, "re-loaded from disk")
    assert again.search(q, k) == (scores, passages, db_ids)
