"""GPU: IndexPQ (faiss.IndexPQ(d, M, 8, metric), contriever/src/index.py:19) through the C-ABI against the CPU oracle.

The oracle needs no flat-PQ entry point: with ONE list, a zero centroid and nprobe 1, orc.ivfpq_search IS FAISS 1.8.0's IndexPQ —
inner product: dis0 = <q, 0> = +0 and 0 + r = r, so the score is the fp32 sum of the M table entries in sub-quantiser order;
L2 (metric=1): q - 0 = q, the squared distance to the decoded vector.  Training is ProductQuantizer::train on the vectors themselves:
pq_train(x[kmeans_sample(n, 256, 256, 1234)], M, 25, 1234); add is pq_encode.  assert_same_results = ids and fp32 scores bit-equal."""
import os
import struct

import numpy as np
import pytest

from util import assert_same_results

pytestmark = pytest.mark.gpu

SEED = 1234
LAYOUTS = {8: [0], 10: [0], 16: [1, 0], 64: [1, 0], 96: [2, 1, 0]}      # pq_layout values an M admits (2 sliced, 1 rotated, 0 granule)


def synth(orc, d, n, ncent=64, nq=0, sigma=0.5):
    x = orc.synth_vectors(d, ncent, 1234, 10000, sigma, 0, n)
    if not nq:
        return x
    return x, orc.synth_queries(d, ncent, 1234, 10000, sigma, n, 999, 0.1, 0, nq)


def oracle_search(orc, cb, codes, q, k, metric=0):
    M, _, dsub = cb.shape
    n = len(codes)
    lm = orc.ListMajor(np.zeros(n, np.int64), np.arange(n), np.ascontiguousarray(codes), 1)
    return orc.ivfpq_search(np.zeros((1, M * dsub), np.float32), cb, lm, np.asarray(q, dtype=np.float32), 1, k, metric=metric)


_CB = {}


def codebooks_for(gpu, orc, d, M):
    """Trained once per (d, M) on the GPU (its bit-equality with the oracle is test_train_matches_oracle's subject)."""
    if (d, M) not in _CB:
        ix = gpu.IndexPQ(d, M, 8, gpu.METRIC_INNER_PRODUCT)
        ix.train(synth(orc, d, 4096))
        _CB[(d, M)] = ix.get_codebooks()
    return _CB[(d, M)]


def make(gpu, orc, d, M, metric=0, layout=None, x=None):
    ix = gpu.IndexPQ(d, M, 8, metric)
    ix.set_codebooks(codebooks_for(gpu, orc, d, M))
    if layout is not None:
        ix.set_param("pq_layout", layout)
        assert ix._get("pq_layout") == layout
    if x is not None:
        ix.add(x)
    return ix


# ------------------------------------------------------------------------------------------ construction, training, add
def test_construction_and_properties(gpu):
    ix = gpu.IndexPQ(64, 8)
    assert ix.metric_type == gpu.METRIC_L2 and ix._get("metric") == 1          # FAISS's default metric for this class
    ix = gpu.IndexPQ(64, 8, 8, gpu.METRIC_INNER_PRODUCT)
    assert not ix.is_trained and ix.ntotal == 0
    assert [ix._get(k) for k in ("kind", "M", "nbits", "code_size", "nshards", "metric", "d")] == [3, 8, 8, 8, 0, 0, 64]
    assert list(ix.list_sizes()) == [0]
    for args, msg in (((64, 8, 4), "nbits"), ((64, 7, 8), "multiple"), ((768, 4, 8), "160")):
        with pytest.raises(RuntimeError, match="rsx error -[16]"):
            gpu.IndexPQ(*args)
    with pytest.raises(RuntimeError, match="rsx error -2"):
        ix.add(np.zeros((4, 64), np.float32))
    with pytest.raises(RuntimeError, match="rsx error -2"):
        ix.search(np.zeros((1, 64), np.float32), 1)


@pytest.mark.parametrize("case", [(64, 8, 5000, "f32"), (768, 96, 20000, "f16"), (768, 16, 20000, "cuda16"), (100, 10, 3000, "cuda32"),
                                  (32, 16, 70000, "f16")], ids=lambda c: "d%d-M%d-n%d-%s" % c)
def test_train_matches_oracle(gpu, orc, case):
    d, M, n, form = case
    x = synth(orc, d, n)
    x32 = x.astype(np.float32)
    sel = orc.kmeans_sample(n, 256, 256, SEED)
    assert len(sel) == min(n, 65536)
    want = orc.pq_train(x32[sel], M, 25, SEED)
    ix = gpu.IndexPQ(d, M, 8, gpu.METRIC_INNER_PRODUCT)
    if form.startswith("cuda"):
        import torch
        xin = torch.from_numpy(x if form == "cuda16" else x32).cuda()
    else:
        xin = x if form == "f16" else x32
    ix.train(xin)
    assert ix.is_trained
    assert np.array_equal(ix.get_codebooks(), want), "codebooks differ from pq_train on the vectors themselves"
    ix.train(xin)          # training twice: the same parameters again
    assert np.array_equal(ix.get_codebooks(), want)


def test_failed_training_leaves_the_handle_usable(gpu, orc):
    d, M, n = 32, 8, 3000
    x = synth(orc, d, n, ncent=8)
    ix = gpu.IndexPQ(d, M, 8, gpu.METRIC_INNER_PRODUCT)
    with pytest.raises(RuntimeError, match="rsx error"):
        ix.train(x[:255])
    assert not ix.is_trained
    ix.train(x)
    want = orc.pq_train(x.astype(np.float32), M, 25, SEED)
    assert np.array_equal(ix.get_codebooks(), want)
    with pytest.raises(RuntimeError, match="rsx error"):
        ix.train(x[:100])
    assert ix.is_trained and np.array_equal(ix.get_codebooks(), want)
    ix.add(x)
    q = x[:5]
    assert_same_results(*ix.search(q, 3), *oracle_search(orc, want, orc.pq_encode(want, x.astype(np.float32)), q, 3), "after failed trainings")


@pytest.mark.parametrize("M,layout", [(8, 0), (16, 1), (64, 1), (96, 2), (96, 1), (96, 0)])
def test_add_in_one_piece_and_in_several(gpu, orc, M, layout):
    d, n = (64 if M <= 16 else 768), 9000
    x = synth(orc, d, n)
    cb = codebooks_for(gpu, orc, d, M)
    want = orc.pq_encode(cb, x.astype(np.float32))
    one = make(gpu, orc, d, M, layout=layout, x=x)
    parts = make(gpu, orc, d, M, layout=layout)
    import torch
    for a, b, form in ((0, 1, "f16"), (1, 700, "f32"), (700, 701, "cuda"), (701, 5000, "f16"), (5000, n, "f32")):      # across capacity growths
        piece = x[a:b] if form == "f16" else x[a:b].astype(np.float32) if form == "f32" else torch.from_numpy(x[a:b]).cuda()
        parts.add(piece)
    for ix in (one, parts):
        codes, ids = ix.get_list(0)
        assert ix.ntotal == n and list(ix.list_sizes()) == [n]
        assert np.array_equal(ids, np.arange(n)) and np.array_equal(codes, want)
    rec = one.reconstruct_n(10, 5)
    assert rec.shape == (5, d)
    assert np.array_equal(rec[2, :d // M], cb[0][want[12, 0]]) and np.array_equal(rec[4, -(d // M):], cb[M - 1][want[14, M - 1]])


# ------------------------------------------------------------------------------------------ search vs oracle, inner product
# every value of k in {1, 10, 100, 1000, 4096} and of nq in {1, 7, 64, 1024} at least once per layout; n not a multiple of any tile
SEARCH_CASES = []
for _M, _lays in LAYOUTS.items():
    for _lay in _lays:
        _d = 100 if _M == 10 else 64 if _M <= 16 else 768
        _n = 20011 if _d == 768 else 50021
        SEARCH_CASES.append((_M, _lay, _d, _n, ((1, 1024), (10, 7), (100, 64), (1000, 1), (4096, 7), (10, 1024))))


@pytest.mark.parametrize("M,layout,d,n,kq", SEARCH_CASES, ids=lambda v: str(v) if isinstance(v, int) else "kq")
def test_search_matches_oracle_ip(gpu, orc, M, layout, d, n, kq):
    x, q = synth(orc, d, n, nq=1024)
    ix = make(gpu, orc, d, M, layout=layout, x=x)
    cb = ix.get_codebooks()
    codes, _ = ix.get_list(0)
    ix.set_param("profile", 1)
    for k, nq in kq:
        Dr, Ir = oracle_search(orc, cb, codes, q[:nq], k)
        assert_same_results(*ix.search(q[:nq], k), Dr, Ir, f"M={M} layout={layout} k={k} nq={nq}")
    if layout != 0 and M in (16, 64, 96):
        assert ix.get_timing("pq_flat_stages") > 0, "the block layouts take the staged scan"
        ix.set_param("profile", 1)
        ix.set_param("pq_flat_first", 2048)                             # several stages on this small index too
        for k, nq in ((10, 1024), (1000, 7)):
            Dr, Ir = oracle_search(orc, cb, codes, q[:nq], k)
            assert_same_results(*ix.search(q[:nq], k), Dr, Ir, f"M={M} layout={layout} k={k} nq={nq}, first stage of 2048 rows")
        assert ix.get_timing("pq_flat_stages") >= 6
        ix.set_param("pq_flat_first", 0)
    import torch
    Dt, It = ix.search(torch.from_numpy(q[:64]).cuda(), 10)            # CUDA tensors in, CUDA tensors out
    Dr, Ir = oracle_search(orc, cb, codes, q[:64], 10)
    assert Dt.is_cuda and It.is_cuda
    assert_same_results(Dt.cpu().numpy(), It.cpu().numpy(), Dr, Ir, "CUDA tensor queries")
    assert_same_results(*ix.search(q[:64].astype(np.float32), 10), Dr, Ir, "fp32 queries")


@pytest.mark.parametrize("M,layout", [(16, 1), (64, 1), (96, 2), (8, 0)])
def test_small_indexes_padding_empty_reset(gpu, orc, M, layout):
    d = 64 if M <= 16 else 768
    x, q = synth(orc, d, 6000, nq=64)
    ix = make(gpu, orc, d, M, layout=layout)
    cb = ix.get_codebooks()
    D, I = ix.search(q[:3], 5)                                          # empty index
    assert (I == -1).all() and np.isneginf(D).all()
    for n, k in ((7, 10), (7, 4096), (100, 100), (1500, 10), (4095, 1000), (6000, 10)):      # n < k: padding; n below the pre-pass sample
        ix.reset()
        assert ix.ntotal == 0
        ix.add(x[:n])
        codes, ids = ix.get_list(0)
        assert np.array_equal(ids, np.arange(n))
        Dr, Ir = oracle_search(orc, cb, codes, q, k)
        D, I = ix.search(q, k)
        assert_same_results(D, I, Dr, Ir, f"M={M} n={n} k={k}")
        if n < k:
            assert (I[:, n:] == -1).all() and np.isneginf(D[:, n:]).all() and (I[:, :n] >= 0).all()


# ------------------------------------------------------------------------------------------ the staged route itself
def _staged_index(gpu, orc):
    d, M, n, nq = 64, 16, 300_000, 1024
    x, q = synth(orc, d, n, ncent=256, nq=nq)
    ix = make(gpu, orc, d, M, layout=1, x=x)
    codes, _ = ix.get_list(0)
    return ix, ix.get_codebooks(), codes, q


def test_staged_route_stages_splits_and_exact_mode(gpu, orc):
    ix, cb, codes, q = _staged_index(gpu, orc)
    k = 10
    Dr, Ir = oracle_search(orc, cb, codes, q, k)
    ix.set_param("profile", 2)
    D, I = ix.search(q, k)
    assert_same_results(D, I, Dr, Ir, "staged scan")
    stages, fast, fb = (ix.get_timing(t) for t in ("pq_flat_stages", "fast_queries", "fallback_queries"))
    print(f"stages {stages} fast {fast} fallback {fb} cand_keys {ix.get_timing('cand_keys')} max {ix.get_timing('cand_keys_max')}")
    assert stages >= 3, "300 000 rows are at least three stages at the default schedule"
    assert fast == len(q)
    for s in range(0, len(q), 256):                                     # a split of the batch into four
        assert_same_results(*ix.search(q[s:s + 256], k), Dr[s:s + 256], Ir[s:s + 256], f"split at {s}")
    for key, v in (("pq_flat_growth", 100), ("pq_flat_first", 4096), ("pq_flat_max_stages", 2), ("pq_flat_max_stages", 1)):   # the schedule never changes a result
        ix.set_param("profile", 1)
        ix.set_param(key, v)
        assert_same_results(*ix.search(q, k), Dr, Ir, f"{key}={v}")
        if key == "pq_flat_max_stages":
            assert ix.get_timing("pq_flat_stages") <= max(v, 1) + 1
    ix.set_param("pq_flat_growth", 0); ix.set_param("pq_flat_first", 0); ix.set_param("pq_flat_max_stages", 0)
    D100r, I100r = oracle_search(orc, cb, codes, q[:128], 1000)
    assert_same_results(*ix.search(q[:128], 1000), D100r, I100r, "staged scan, k = 1000")
    ix.set_param("profile", 1)
    ix.set_param("pq_fast", 0)                                          # the exact route
    assert_same_results(*ix.search(q[:64], k), Dr[:64], Ir[:64], "pq_fast = 0")
    assert ix.get_timing("pq_flat_stages") == 0
    ix.set_param("pq_fast", 1); ix.set_param("scan_kernel", 2)
    assert_same_results(*ix.search(q[:64], k), Dr[:64], Ir[:64], "scan_kernel = 2")


def test_staged_route_with_every_capacity_starved(gpu, orc):
    ix, cb, codes, q = _staged_index(gpu, orc)
    k = 10
    Dr, Ir = oracle_search(orc, cb, codes, q, k)
    ix.set_param("profile", 1)
    ix.set_param("pq_log_cap", 1)                                       # one key per survivor log: nearly every run loses keys
    ix.set_param("pq_fast_kp", 16)                                      # the smallest K'
    ix.set_param("pq_final_tab", 0)
    D, I = ix.search(q, k)
    fb = ix.get_timing("fallback_queries")
    print(f"starved: fallback_queries {fb} of {len(q)}, overflow {ix.get_timing('fallback_overflow_queries')}")
    assert fb > 0, "starved logs must show as fallbacks"
    assert_same_results(D, I, Dr, Ir, "starved capacities")
    ix.set_param("profile", 1)
    ix.set_param("pq_final_tab", 1)
    assert_same_results(*ix.search(q, k), Dr, Ir, "starved logs, finalize from the row")
    assert ix.get_timing("fallback_queries") > 0


# ------------------------------------------------------------------------------------------ hostile orders
@pytest.mark.parametrize("order", ["ascending", "descending", "identical", "two_sources"])
def test_hostile_orders(gpu, orc, order):
    d, M, n, nq, k = 64, 16, 150_000, 64, 10
    x, q = synth(orc, d, n, ncent=256, nq=nq)
    if order in ("ascending", "descending"):                            # sorted by the exact score of query 0: early thresholds useless / everything early
        s = x.astype(np.float32) @ q[0].astype(np.float32)
        o = np.argsort(s, kind="stable")
        x = x[o if order == "ascending" else o[::-1]]
    elif order == "identical":
        x = np.repeat(x[:1], 40_000, axis=0)                            # every score ties: ids ascending
    else:
        x2 = orc.synth_vectors(d, 16, 77, 88, 2.0, 0, n // 2)           # another mixture, added after the first
        x = np.concatenate([x[:n // 2], x2])
    ix = make(gpu, orc, d, M, layout=1)
    if order == "two_sources":
        ix.add(x[:n // 2]); ix.add(x[n // 2:])
    else:
        ix.add(x)
    codes, _ = ix.get_list(0)
    ix.set_param("profile", 2)
    for kk in (k, 100):
        Dr, Ir = oracle_search(orc, ix.get_codebooks(), codes, q, kk)
        D, I = ix.search(q, kk)
        assert_same_results(D, I, Dr, Ir, f"{order} k={kk}")
    print(f"{order}: stages {ix.get_timing('pq_flat_stages')} fallback {ix.get_timing('fallback_queries')} cand_keys_max {ix.get_timing('cand_keys_max')}")
    if order == "identical":
        assert np.array_equal(I[0], np.arange(100))


# ------------------------------------------------------------------------------------------ L2
@pytest.mark.parametrize("M,d,n", [(8, 64, 5000), (96, 768, 20000), (64, 768, 20000), (10, 100, 3000), (16, 64, 30000)])
def test_l2_matches_oracle(gpu, orc, M, d, n):
    x, q = synth(orc, d, n, nq=64)
    for layout in LAYOUTS[M]:
        ix = make(gpu, orc, d, M, metric=gpu.METRIC_L2, layout=layout, x=x)
        codes, _ = ix.get_list(0)
        for k, nq in ((10, 64), (100, 7), (1, 1)):
            Dr, Ir = oracle_search(orc, ix.get_codebooks(), codes, q[:nq], k, metric=1)
            assert_same_results(*ix.search(q[:nq], k), Dr, Ir, f"L2 M={M} layout={layout} k={k}")
        ix.reset()
        ix.add(x[:3])
        D, I = ix.search(q[:2], 5)
        assert (I[:, 3:] == -1).all() and np.isposinf(D[:, 3:]).all()
    # the distances are those to the decoded vectors
    rec = ix.reconstruct_n(0, 3).astype(np.float64)
    ref = ((q[:2].astype(np.float64)[:, None, :] - rec[None]) ** 2).sum(-1)
    assert np.allclose(np.sort(ref, axis=1), D[:, :3], rtol=1e-5)


# ------------------------------------------------------------------------------------------ the one-list IVF-PQ emulation
@pytest.mark.parametrize("metric", [0, 1])
def test_equals_a_one_list_ivfpq(gpu, orc, metric):
    d, M, n = 768, 64, 30000
    x, q = synth(orc, d, n, nq=256)
    cb = codebooks_for(gpu, orc, d, M)
    ix = make(gpu, orc, d, M, metric=metric, x=x)
    em = gpu.IndexIVFPQ(gpu.IndexFlatIP(d), d, 1, M, 8, metric)
    em.set_centroids(np.zeros((1, d), np.float32)); em.set_codebooks(cb)
    em.add(x); em.nprobe = 1
    assert np.array_equal(ix.get_list(0)[0], em.get_list(0)[0])
    for k in (10, 200):
        D, I = ix.search(q, k)
        De, Ie = em.search(q, k)
        assert_same_results(D, I, De, Ie, f"one-list IVF-PQ, metric {metric}, k={k}")


# ------------------------------------------------------------------------------------------ persistence
def test_save_load_and_faiss_file(gpu, orc, tmp_path, monkeypatch):
    d, M, n = 768, 96, 12000
    x, q = synth(orc, d, n, nq=64)
    ix = make(gpu, orc, d, M, x=x)
    codes, ids = ix.get_list(0)
    D, I = ix.search(q, 10)
    p1, p2 = str(tmp_path / "pq.rsx"), str(tmp_path / "pq.faiss")
    gpu.write_index(ix, p1)
    monkeypatch.setenv("RSX_INDEX_FORMAT", "faiss")
    gpu.write_index(ix, p2)
    monkeypatch.delenv("RSX_INDEX_FORMAT")
    assert open(p1, "rb").read(4) == b"RSX1" and open(p2, "rb").read(4) == b"IxPq"
    hdr = open(p2, "rb").read(4 + 4 + 8)
    assert struct.unpack("<iq", hdr[4:]) == (d, n)
    for path in (p1, p2):
        ld = gpu.read_index(path)
        assert type(ld) is gpu.IndexPQ and ld._get("kind") == 3 and ld.ntotal == n and ld.is_trained and ld.M == M and ld.d == d
        c2, i2 = ld.get_list(0)
        assert np.array_equal(c2, codes) and np.array_equal(i2, ids) and np.array_equal(ld.get_codebooks(), ix.get_codebooks())
        assert_same_results(*ld.search(q, 10), D, I, f"loaded from {os.path.basename(path)}")
        ld.add(x[:100])                                                 # a loaded index keeps counting ids
        assert np.array_equal(ld.get_list(0)[1], np.arange(n + 100))
    with pytest.raises(RuntimeError, match="rsx error -6"):
        gpu.read_index(p1, devices=[0, 0])                              # no sharded form


def test_contriever_indexer_call_sequence(gpu, orc, tmp_path):
    """contriever/src/index.py Indexer with n_subquantizers > 0, its calls written out: IndexPQ(vector_sz, n_subquantizers, n_bits,
    METRIC_INNER_PRODUCT), index_data (train when not is_trained, add float32), search_knn in batches of 2048, serialize /
    deserialize_from through write_index / read_index."""
    faiss = gpu
    d, M, n = 768, 64, 9000
    x, q = synth(orc, d, n, nq=2500)
    index = faiss.IndexPQ(d, M, 8, faiss.METRIC_INNER_PRODUCT)
    emb = x.astype("float32")
    if not index.is_trained:
        index.train(emb)
    index.add(emb[:5000]); index.add(emb[5000:])
    qv = q.astype("float32")
    res = [index.search(qv[b:b + 2048], 20) for b in range(0, len(qv), 2048)]
    D, I = np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])
    codes, _ = index.get_list(0)
    assert_same_results(D, I, *oracle_search(orc, index.get_codebooks(), codes, qv, 20), "contriever Indexer sequence")
    path = str(tmp_path / "index.faiss")
    faiss.write_index(index, path)
    index2 = faiss.read_index(path)
    assert index2.ntotal == n == index.ntotal
    assert_same_results(*index2.search(qv[:2048], 20), D[:2048], I[:2048], "after deserialize_from")


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_usable(gpu, orc):
    import ctypes
    import torch
    d, M, n = 64, 16, 20000
    x, q = synth(orc, d, n, nq=64)
    ix = make(gpu, orc, d, M, x=x)
    codes, _ = ix.get_list(0)
    Dr, Ir = oracle_search(orc, ix.get_codebooks(), codes, q, 10)
    sel = gpu.IDSelectorRange(0, 100)
    L = gpu.lib()

    def refused(code, f):
        with pytest.raises(RuntimeError, match=f"rsx error {code}: .*IndexPQ"):
            f()
        assert_same_results(*ix.search(q, 10), Dr, Ir, "search after a refusal")
        assert ix.ntotal == n

    refused(-6, lambda: ix.search(q, 10, params=gpu.SearchParameters(sel=sel)))
    refused(-6, lambda: ix.search_prepass(torch.from_numpy(q).cuda(), 10, params=gpu.SearchParameters(sel=sel)))
    refused(-6, lambda: ix.remove_ids(sel))
    refused(-6, lambda: ix.add_with_ids(x[:4], np.arange(4) + 7))
    refused(-1, lambda: ix.set_param("add_list_mod", 2))
    refused(-1, lambda: gpu._check(L.rsx_set_nprobe(ix._h, 4)))
    lab = np.zeros(4, np.int64)
    refused(-1, lambda: gpu._check(L.rsx_assign(ix._h, ctypes.c_int64(4), x[:4].ctypes.data_as(ctypes.c_void_p), 1, lab.ctypes.data_as(ctypes.c_void_p))))
    cnt = np.array([n], np.int64)
    refused(-1, lambda: gpu._check(L.rsx_reserve_lists(ix._h, cnt.ctypes.data_as(ctypes.c_void_p))))
    cen = np.zeros((1, d), np.float32)
    refused(-1, lambda: gpu._check(L.rsx_set_centroids(ix._h, cen.ctypes.data_as(ctypes.c_void_p))))
    refused(-1, lambda: gpu._check(L.rsx_get_centroids(ix._h, cen.ctypes.data_as(ctypes.c_void_p))))
    h = ctypes.c_void_p()
    devs = (ctypes.c_int * 2)(0, 0)
    with pytest.raises(RuntimeError, match="rsx error -6"):
        gpu._check(L.rsx_sharded_create(3, d, 1, M, 8, 0, 2, devs, ctypes.byref(h)))
    # an unfiltered search through the parameter and the two-call forms is served; the two-call search has no thresholds to hand out
    assert_same_results(*ix.search(q, 10, params=gpu.SearchParameters()), Dr, Ir, "params without a selector")
    assert ix.search_prepass(torch.from_numpy(q).cuda(), 10) is None
    Dt, It = ix.search_scan()
    assert_same_results(Dt.cpu().numpy(), It.cpu().numpy(), Dr, Ir, "two-call search")
    with pytest.raises(RuntimeError, match="rsx error -1"):
        ix.set_param("pq_layout", 0)                                    # only before the first add
    with pytest.raises(RuntimeError, match="rsx error -6"):
        ix.search(q, 4097)
