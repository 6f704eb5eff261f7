"""GPU: IndexPQ at 10M x 768 (the bench generator's mixture: NC 4096, seeds 1234 / 10000 / 999), M = 96 and M = 64 in their default
layouts, inner product, batch 1024 — the staged filtered scan at the size it was built for.

Each: the eight SAMPLE queries of the timed batch bit-equal (ids AND fp32 scores) to the CPU oracle run on the exported codes, for
k = 10 and — as part of the whole batch — k = 1000; the whole batch invariant under a split into four; and ZERO fallbacks at k = 10:
the same tables and certificate clear every query of the 100M IVF-PQ test on this data, so a fallback here would be a fault of the
threshold schedule or of a capacity (a re-run query is still compared with the oracle: the condition only keeps the test from passing
on the slow route)."""
import numpy as np
import pytest

from util import assert_same_results

pytestmark = pytest.mark.gpu

D, NC, SC, SX, SQ = 768, 4096, 1234, 10000, 999
SAMPLE = [0, 1, 255, 256, 511, 640, 777, 1023]


@pytest.mark.parametrize("M", [96, 64])
def test_indexpq_10M_batch_1024(gpu, orc, M):
    import torch
    dev = torch.device("cuda", 0)
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * (1 << 30):
        pytest.skip("needs 16 GB of free HBM")
    n, nq = 10_000_000, 1024
    ix = gpu.IndexPQ(D, M, 8, gpu.METRIC_INNER_PRODUCT)
    xt = torch.empty((65536, D), dtype=torch.float16, device=dev)
    gpu.synth_vectors(D, NC, SC, SX, 0.5, 0, 65536, out=xt)
    ix.train(xt); del xt
    buf = torch.empty((1_000_000, D), dtype=torch.float16, device=dev)
    for c0 in range(0, n, buf.shape[0]):
        gpu.synth_vectors(D, NC, SC, SX, 0.5, c0, buf.shape[0], out=buf); ix.add(buf)
    del buf
    assert ix.ntotal == n and ix._get("pq_layout") == (2 if M == 96 else 1)
    q = torch.empty((nq, D), dtype=torch.float16, device=dev)
    gpu.synth_queries(D, NC, SC, SX, 0.5, n, SQ, 0.1, 0, nq, out=q)
    ix.set_param("profile", 2)
    Dg, Ig = ix.search(q, 10)
    stats = {t: ix.get_timing(t) for t in ("pq_flat_stages", "fast_queries", "fallback_queries", "cand_keys", "cand_keys_max", "total", "scan")}
    print(f"M={M} k=10: {stats}")
    assert stats["pq_flat_stages"] >= 3 and stats["fast_queries"] == nq
    assert stats["fallback_queries"] == 0, "the staged scan must settle every query of this data by itself"
    for s in range(0, nq, 256):
        Ds, Is = ix.search(q[s:s + 256], 10)
        assert torch.equal(Ds, Dg[s:s + 256]) and torch.equal(Is, Ig[s:s + 256]), f"batch split at {s} changes the result"
    codes, ids = ix.get_list(0)
    assert np.array_equal(ids[[0, 1, n // 2, n - 1]], [0, 1, n // 2, n - 1])
    cb = ix.get_codebooks()
    qs = q[SAMPLE].cpu().numpy().astype(np.float32)
    lm = orc.ListMajor(np.zeros(1, np.int64), np.zeros(1, np.int64), codes[:1], 1)       # (one list: no argsort over 10M entries)
    lm.list_off = np.array([0, n], np.int64); lm.ids = ids; lm.payload = codes
    zero = np.zeros((1, D), np.float32)
    Do, Io = orc.ivfpq_search(zero, cb, lm, qs, 1, 1000)
    assert_same_results(Dg.cpu().numpy()[SAMPLE], Ig.cpu().numpy()[SAMPLE], Do[:, :10], Io[:, :10], f"10M IndexPQ M={M} k = 10 vs CPU oracle (8 queries)")
    ix.set_param("profile", 2)
    Dk, Ik = ix.search(q, 1000)
    print(f"M={M} k=1000: " + str({t: ix.get_timing(t) for t in ("pq_flat_stages", "fallback_queries", "cand_keys", "cand_keys_max", "total")}))
    assert_same_results(Dk.cpu().numpy()[SAMPLE], Ik.cpu().numpy()[SAMPLE], Do, Io, f"10M IndexPQ M={M} k = 1000 (whole batch) vs CPU oracle")


def test_indexpq_one_list_beyond_2GiB_of_codes(gpu, orc):
    """40M x 64 bytes = 2.56 GB in ONE list: past what the list-wide scans' 32-bit byte offsets reach.  The staged scan hands every work item
    its tile as a list of its own and the exact scan addresses rows with 64-bit offsets, so both must still equal the oracle — also for
    the queries whose neighbours sit in the upper part of the list; the routes that cannot are refused, never wrong."""
    import torch
    dev = torch.device("cuda", 0)
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * (1 << 30):
        pytest.skip("needs 16 GB of free HBM")
    n, M, nq, k = 40_000_000, 64, 1024, 10
    assert n * M > (1 << 31)
    ix = gpu.IndexPQ(D, M, 8, gpu.METRIC_INNER_PRODUCT)
    xt = torch.empty((65536, D), dtype=torch.float16, device=dev)
    gpu.synth_vectors(D, NC, SC, SX, 0.5, 0, 65536, out=xt)
    ix.train(xt); del xt
    buf = torch.empty((1_000_000, D), dtype=torch.float16, device=dev)
    for c0 in range(0, n, buf.shape[0]):
        gpu.synth_vectors(D, NC, SC, SX, 0.5, c0, buf.shape[0], out=buf); ix.add(buf)
    del buf
    q = torch.empty((nq, D), dtype=torch.float16, device=dev)
    gpu.synth_queries(D, NC, SC, SX, 0.5, n, SQ, 0.1, 0, nq, out=q)
    ix.set_param("profile", 1)
    Dg, Ig = ix.search(q, k)
    assert ix.get_timing("pq_flat_stages") >= 3 and ix.get_timing("fallback_queries") == 0
    Ih = Ig.cpu().numpy()
    # (16 % of the rows lie beyond the 2 GiB mark, and a query's best neighbour is the stored vector it was generated from: ~165 of 1024)
    beyond = np.nonzero(Ih[:, 0] >= (1 << 31) // M)[0]
    assert len(beyond) > 32, "part of the batch must have its best neighbour beyond the 2 GiB mark"
    codes, ids = ix.get_list(0)
    lm = orc.ListMajor(np.zeros(1, np.int64), np.zeros(1, np.int64), codes[:1], 1)
    lm.list_off = np.array([0, n], np.int64); lm.ids = ids; lm.payload = codes
    sample = SAMPLE + [int(i) for i in beyond[:8]]                      # the usual eight and eight whose answer starts beyond the mark
    qs = q[sample].cpu().numpy().astype(np.float32)
    Do, Io = orc.ivfpq_search(np.zeros((1, D), np.float32), ix.get_codebooks(), lm, qs, 1, k)
    assert_same_results(Dg.cpu().numpy()[sample], Ih[sample], Do, Io, "40M IndexPQ, staged scan vs CPU oracle (16 queries)")
    ix.set_param("pq_fast", 0)                                          # the exact scan
    De, Ie = ix.search(q[sample], k)
    assert_same_results(De.cpu().numpy(), Ie.cpu().numpy(), Do, Io, "40M IndexPQ, exact scan vs CPU oracle")
    ix.set_param("pq_fast", 1); ix.set_param("pq_filter", 0)            # the list-wide fast scan: refused at this size
    with pytest.raises(RuntimeError, match="rsx error -6: IndexPQ"):
        ix.search(q[:8], k)
    ix.set_param("pq_filter", 1)
    Da, Ia = ix.search(q, k)
    assert torch.equal(Da, Dg) and torch.equal(Ia, Ig), "the handle serves the staged scan again after the refusal"
