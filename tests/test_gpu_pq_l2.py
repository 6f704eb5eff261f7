"""GPU: an L2 IndexPQ (faiss.IndexPQ's default metric) takes the staged 8-bit scan and still equals the CPU oracle bit for bit.

The reference is test_gpu_pq.py's: orc.ivfpq_search with ONE list, a zero centroid and metric=1 IS FAISS 1.8.0's IndexPQ under L2
(q - 0 = q: the squared distance to the decoded vector, fmaf chains per sub-quantiser, summed in m order).  assert_same_results =
ids and fp32 distances bit-equal; there is no tolerance in this file.  The route is read from the handle's own counters
(set_param("profile", 1) clears them): pq_flat_stages > 0 = pq_staged_scan served the batch.

Fallback cap: the exact re-run of flagged queries is always right, so a broken table builder could hide behind it.  Where the route is
not starved on purpose at most 5 % of a search's queries may be re-run (fallback_queries) and none for an overflowed candidate row or
survivor log (fallback_overflow_queries); tests/test_pq_l2_band_host.py shows on the CPU that these inputs sit far inside a row."""
import os

import numpy as np
import pytest

from test_gpu_pq import codebooks_for, make, oracle_search, synth
from util import assert_same_results

pytestmark = pytest.mark.gpu


def counters(ix):
    return {t: ix.get_timing(t) for t in ("pq_flat_stages", "fast_queries", "fallback_queries", "fallback_overflow_queries")}


def search_checked(ix, orc, cb, codes, q, k, what, capped=True, staged=True):
    """One search against the oracle (metric=1) with the handle's counters cleared before it; returns the counters."""
    Dr, Ir = oracle_search(orc, cb, codes, q, k, metric=1)
    ix.set_param("profile", 1)
    D, I = ix.search(q, k)
    c = counters(ix)
    print(f"{what}: stages {c['pq_flat_stages']:.0f} fast {c['fast_queries']:.0f} fallback {c['fallback_queries']:.0f} of {len(q)} "
          f"(overflow {c['fallback_overflow_queries']:.0f})")
    assert_same_results(D, I, Dr, Ir, what)
    if staged is not None:
        assert (c["pq_flat_stages"] > 0) == staged, f"{what}: pq_flat_stages = {c['pq_flat_stages']}"
    if capped:
        assert c["fallback_queries"] <= 0.05 * len(q), f"{what}: {c['fallback_queries']:.0f} of {len(q)} queries re-run exactly"
        assert c["fallback_overflow_queries"] == 0, f"{what}: a candidate row or survivor log overflowed"
    return c


# ------------------------------------------------------------------------------------------ 1. route + parity
@pytest.mark.parametrize("M,layout", [(16, 1), (64, 1), (96, 2), (96, 1)])
def test_route_and_parity(gpu, orc, M, layout):
    d = 64 if M <= 16 else 768
    n = 20011 if d == 768 else 50021
    x, q = synth(orc, d, n, nq=1024)
    ix = make(gpu, orc, d, M, metric=gpu.METRIC_L2, layout=layout, x=x)
    assert ix.metric_type == gpu.METRIC_L2
    cb = ix.get_codebooks()
    codes, _ = ix.get_list(0)
    stages = 0
    for k, nq in ((1, 1024), (10, 7), (100, 64), (1000, 1), (4096, 7), (10, 1024)):
        c = search_checked(ix, orc, cb, codes, q[:nq], k, f"L2 M={M} layout={layout} k={k} nq={nq}", staged=True if k <= 100 else None)
        stages += c["pq_flat_stages"]
    assert stages > 0, "an L2 IndexPQ in a block layout takes the staged scan"
    ix.set_param("pq_flat_first", 2048)                                 # several stages on this small index too
    stages = 0
    for k, nq in ((10, 1024), (1000, 7)):
        stages += search_checked(ix, orc, cb, codes, q[:nq], k, f"L2 M={M} layout={layout} k={k} nq={nq}, first stage of 2048 rows",
                                 staged=None)["pq_flat_stages"]
    assert stages >= 6
    ix.set_param("pq_flat_first", 0)
    import torch
    Dr, Ir = oracle_search(orc, cb, codes, q[:64], 10, metric=1)
    Dt, It = ix.search(torch.from_numpy(q[:64]).cuda(), 10)             # CUDA tensors in, CUDA tensors out
    assert Dt.is_cuda and It.is_cuda
    assert_same_results(Dt.cpu().numpy(), It.cpu().numpy(), Dr, Ir, "CUDA tensor queries")
    assert q.dtype == np.float16
    assert_same_results(*ix.search(q[:64], 10), Dr, Ir, "fp16 queries")
    assert_same_results(*ix.search(q[:64].astype(np.float32), 10), Dr, Ir, "fp32 queries")


# ------------------------------------------------------------------------------------------ 2. stages at size
def _staged_index(gpu, orc):
    d, M, n, nq = 64, 16, 300_000, 1024
    x, q = synth(orc, d, n, ncent=256, nq=nq)
    ix = make(gpu, orc, d, M, metric=gpu.METRIC_L2, layout=1, x=x)
    codes, _ = ix.get_list(0)
    return ix, ix.get_codebooks(), codes, q


def test_stages_splits_schedule_and_exact_mode(gpu, orc):
    ix, cb, codes, q = _staged_index(gpu, orc)
    for k in (10, 1000):
        c = search_checked(ix, orc, cb, codes, q, k, f"staged L2 scan, k={k}")
        assert c["pq_flat_stages"] >= 3, "300 000 rows are at least three stages at the default schedule"
        assert c["fast_queries"] == len(q)
    k = 10
    Dr, Ir = oracle_search(orc, cb, codes, q, k, metric=1)
    for s in range(0, len(q), 256):                                     # a split of the batch into four
        assert_same_results(*ix.search(q[s:s + 256], k), Dr[s:s + 256], Ir[s:s + 256], f"split at {s}")
    for key, v in (("pq_flat_growth", 100), ("pq_flat_first", 4096), ("pq_flat_max_stages", 2), ("pq_flat_max_stages", 1)):   # the schedule never changes a result
        ix.set_param("profile", 1)
        ix.set_param(key, v)
        assert_same_results(*ix.search(q, k), Dr, Ir, f"{key}={v}")
        assert ix.get_timing("pq_flat_stages") > 0
        if key == "pq_flat_max_stages":
            assert ix.get_timing("pq_flat_stages") <= max(v, 1) + 1
    ix.set_param("pq_flat_growth", 0); ix.set_param("pq_flat_first", 0); ix.set_param("pq_flat_max_stages", 0)
    ix.set_param("profile", 1)
    ix.set_param("pq_fast", 0)                                          # the exact route
    assert_same_results(*ix.search(q[:64], k), Dr[:64], Ir[:64], "pq_fast = 0")
    assert ix.get_timing("pq_flat_stages") == 0
    ix.set_param("pq_fast", 1); ix.set_param("scan_kernel", 2)
    assert_same_results(*ix.search(q[:64], k), Dr[:64], Ir[:64], "scan_kernel = 2")
    assert ix.get_timing("pq_flat_stages") == 0
    ix.set_param("scan_kernel", 0)
    assert_same_results(*ix.search(q[:64], k), Dr[:64], Ir[:64], "back on the staged scan")
    assert ix.get_timing("pq_flat_stages") > 0


# ------------------------------------------------------------------------------------------ 3. starved capacities: the re-run path under L2
def test_every_capacity_starved(gpu, orc):
    ix, cb, codes, q = _staged_index(gpu, orc)
    k = 10
    ix.set_param("pq_log_cap", 1)                                       # one key per survivor log: nearly every run loses keys
    ix.set_param("pq_fast_kp", 16)                                      # the smallest K'
    for final_tab in (0, 1):
        ix.set_param("pq_final_tab", final_tab)
        c = search_checked(ix, orc, cb, codes, q, k, f"starved capacities, pq_final_tab={final_tab}", capped=False)
        assert c["fallback_queries"] > 0, "starved logs must show as fallbacks"


# ------------------------------------------------------------------------------------------ 4. hostile orders, signed zero
@pytest.mark.parametrize("order", ["ascending", "descending", "identical", "two_sources"])
def test_hostile_orders(gpu, orc, order):
    d, M, n, nq, k = 64, 16, 150_000, 64, 10
    x, q = synth(orc, d, n, ncent=256, nq=nq)
    if order in ("ascending", "descending"):                            # sorted by the exact DISTANCE to query 0: everything early / early thresholds useless
        s = ((x.astype(np.float32) - q[0].astype(np.float32)) ** 2).sum(axis=1)
        o = np.argsort(s, kind="stable")
        x = x[o if order == "ascending" else o[::-1]]
    elif order == "identical":
        x = np.repeat(x[:1], 40_000, axis=0)                            # every distance ties: ids ascending
    else:
        x2 = orc.synth_vectors(d, 16, 77, 88, 2.0, 0, n // 2)           # another mixture, added after the first
        x = np.concatenate([x[:n // 2], x2])
    ix = make(gpu, orc, d, M, metric=gpu.METRIC_L2, layout=1)
    if order == "two_sources":
        ix.add(x[:n // 2]); ix.add(x[n // 2:])
    else:
        ix.add(x)
    codes, _ = ix.get_list(0)
    for kk in (k, 100):                                                 # (a sorted order may honestly fill a row: the count is printed, not capped)
        search_checked(ix, orc, ix.get_codebooks(), codes, q, kk, f"{order} k={kk}", capped=False)
    if order == "identical":
        D, I = ix.search(q, 100)
        assert np.array_equal(I[0], np.arange(100)) and (D[0] == D[0, 0]).all()


def test_signed_zero_distance(gpu, orc):
    """Queries that ARE decoded vectors: the distance to every row with the same codes is exactly 0 — a negated sum of -0 entries on the
    way — and must come out +0.0f, the ties in id order."""
    d, M, n = 64, 16, 30_000
    x = synth(orc, d, n)
    ix = make(gpu, orc, d, M, metric=gpu.METRIC_L2, layout=1, x=x)
    ix.add(x[:16]); ix.add(x[:16])                                      # two more copies of the first 16 rows: ids n + i and n + 16 + i
    q = ix.reconstruct_n(0, 16)
    assert q.dtype == np.float32
    codes, _ = ix.get_list(0)
    assert np.array_equal(codes[:16], codes[n:n + 16]) and np.array_equal(codes[:16], codes[n + 16:])
    for k in (1, 10, 100):
        Dr, Ir = oracle_search(orc, ix.get_codebooks(), codes, q, k, metric=1)
        ix.set_param("profile", 1)
        D, I = ix.search(q, k)
        assert_same_results(D, I, Dr, Ir, f"decoded vectors as queries, k={k}")
        assert ix.get_timing("pq_flat_stages") > 0
        nz = min(k, 3)
        assert (D[:, :nz] == 0).all() and not np.signbit(D[:, :nz]).any() and not np.signbit(Dr[:, :nz]).any()
        assert (np.diff(I[:, :nz], axis=1) > 0).all(), "ties in id order"
    assert np.array_equal(I[:, 0], np.arange(16))
    ix.set_param("pq_fast", 0)                                          # the exact scan agrees on the sign
    D0, I0 = ix.search(q, 10)
    assert_same_results(D0, I0, *oracle_search(orc, ix.get_codebooks(), codes, q, 10, metric=1), "decoded vectors, pq_fast = 0")
    assert not np.signbit(D0[:, :3]).any()


# ------------------------------------------------------------------------------------------ 5. edges, persistence
@pytest.mark.parametrize("M,layout", [(16, 1), (64, 1), (96, 2)])
def test_small_indexes_padding_empty_reset(gpu, orc, M, layout):
    d = 64 if M <= 16 else 768
    x, q = synth(orc, d, 6000, nq=64)
    ix = make(gpu, orc, d, M, metric=gpu.METRIC_L2, layout=layout)
    cb = ix.get_codebooks()
    D, I = ix.search(q[:3], 5)                                          # empty index
    assert (I == -1).all() and np.isposinf(D).all()
    for n, k in ((7, 10), (7, 4096), (100, 100), (1500, 10), (4095, 1000), (6000, 10)):      # n < k: padding; n below the pre-pass sample
        ix.reset()
        assert ix.ntotal == 0
        ix.add(x[:n])
        codes, ids = ix.get_list(0)
        assert np.array_equal(ids, np.arange(n))
        Dr, Ir = oracle_search(orc, cb, codes, q, k, metric=1)
        ix.set_param("profile", 1)
        D, I = ix.search(q, k)
        assert_same_results(D, I, Dr, Ir, f"L2 M={M} n={n} k={k}")
        if k <= 100:
            assert ix.get_timing("pq_flat_stages") > 0
        if n < k:
            assert (I[:, n:] == -1).all() and np.isposinf(D[:, n:]).all() and (I[:, :n] >= 0).all()


def test_save_load_keeps_the_route(gpu, orc, tmp_path, monkeypatch):
    d, M, n = 768, 96, 12000
    x, q = synth(orc, d, n, nq=64)
    ix = make(gpu, orc, d, M, metric=gpu.METRIC_L2, x=x)
    codes, ids = ix.get_list(0)
    Dr, Ir = oracle_search(orc, ix.get_codebooks(), codes, q, 10, metric=1)
    ix.set_param("profile", 1)
    assert_same_results(*ix.search(q, 10), Dr, Ir, "before saving")
    assert ix.get_timing("pq_flat_stages") > 0
    p1, p2 = str(tmp_path / "pq_l2.rsx"), str(tmp_path / "pq_l2.faiss")
    gpu.write_index(ix, p1)
    monkeypatch.setenv("RSX_INDEX_FORMAT", "faiss")
    gpu.write_index(ix, p2)
    monkeypatch.delenv("RSX_INDEX_FORMAT")
    assert open(p1, "rb").read(4) == b"RSX1" and open(p2, "rb").read(4) == b"IxPq"
    for path in (p1, p2):
        ld = gpu.read_index(path)
        assert type(ld) is gpu.IndexPQ and ld._get("kind") == 3 and ld._get("metric") == 1 and ld.metric_type == gpu.METRIC_L2
        assert ld.ntotal == n and np.array_equal(ld.get_list(0)[0], codes)
        ld.set_param("profile", 1)
        assert_same_results(*ld.search(q, 10), Dr, Ir, f"loaded from {os.path.basename(path)}")
        assert ld.get_timing("pq_flat_stages") > 0, "a loaded L2 IndexPQ takes the staged scan"
        assert ld.get_timing("fallback_overflow_queries") == 0


# ------------------------------------------------------------------------------------------ 6. unchanged neighbours
@pytest.mark.parametrize("M,d,n,layout", [(16, 64, 30000, 0), (96, 768, 20000, 0), (8, 64, 5000, None), (10, 100, 3000, None)])
def test_other_l2_indexpq_settings_keep_the_exact_scan(gpu, orc, M, d, n, layout):
    x, q = synth(orc, d, n, nq=64)
    ix = make(gpu, orc, d, M, metric=gpu.METRIC_L2, layout=layout, x=x)
    codes, _ = ix.get_list(0)
    for k, nq in ((10, 64), (100, 7)):
        search_checked(ix, orc, ix.get_codebooks(), codes, q[:nq], k, f"L2 M={M} layout={layout} k={k}", capped=False, staged=False)


def test_one_list_l2_ivfpq_keeps_the_exact_scan_and_ip_keeps_its_stages(gpu, orc):
    d, M, n = 768, 64, 30000
    x, q = synth(orc, d, n, nq=256)
    cb = codebooks_for(gpu, orc, d, M)
    em = gpu.IndexIVFPQ(gpu.IndexFlatIP(d), d, 1, M, 8, gpu.METRIC_L2)
    em.set_centroids(np.zeros((1, d), np.float32)); em.set_codebooks(cb)
    em.add(x); em.nprobe = 1
    codes, _ = em.get_list(0)
    search_checked(em, orc, cb, codes, q, 10, "one-list L2 IVF-PQ", capped=False, staged=False)
    ip = make(gpu, orc, d, M, metric=gpu.METRIC_INNER_PRODUCT, x=x)
    assert np.array_equal(ip.get_list(0)[0], codes)
    ip.set_param("profile", 1)
    assert_same_results(*ip.search(q, 10), *oracle_search(orc, cb, codes, q, 10), "inner-product IndexPQ on the same data")
    assert ip.get_timing("pq_flat_stages") > 0 and ip.get_timing("fallback_queries") == 0
    l2 = make(gpu, orc, d, M, metric=gpu.METRIC_L2, x=x)
    search_checked(l2, orc, cb, codes, q, 10, "L2 IndexPQ on the same data")
