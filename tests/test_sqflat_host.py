"""CPU: the ABI and Python surface of IndexScalarQuantizer (RSX_KIND_SQ = 5), the numpy restatement of its int8 scan (tests/sqflat_ref.py:
bit budget, planes, bound) checked against every (query, row) pair of the input sets, and the preconditions the GPU tests
(tests/test_gpu_sqflat.py) lean on, asserted from the oracle alone."""
import os
import re

import numpy as np
import pytest

import sq_ref
import sqflat_ref
from conftest import REPO

F32 = np.float32
pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered")      # inf - inf between padded results


# ------------------------------------------------------------------------------------------ 1. ABI and surface
def test_abi_version_kind_and_symbol(rsxlib):
    assert rsxlib.lib().rsx_version() >= 1009
    header = open(os.path.join(REPO, "include", "rsx.h")).read()
    assert re.search(r"RSX_KIND_SQ\s*=\s*5", header)
    assert re.search(r"int\s+rsx_sq_create\(int d, int qtype, int metric, int device, rsx_index_t\*\* out\)", header)
    assert "rsx_sq_create" in rsxlib.ABI_SYMBOLS and getattr(rsxlib.lib(), "rsx_sq_create") is not None


def test_no_cpu_path(rsxlib):
    if rsxlib.get_num_gpus() > 0:
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        rsxlib.IndexScalarQuantizer(16, rsxlib.ScalarQuantizer.QT_8bit, rsxlib.METRIC_INNER_PRODUCT)
    with pytest.raises(RuntimeError, match="no HIP device"):
        rsxlib.index_factory(16, "SQ8")


@pytest.mark.parametrize("qtype", [1, 2, 3, 4, 5, 6])
def test_other_qtypes_are_refused(rsxlib, qtype):
    with pytest.raises(RuntimeError, match="IndexScalarQuantizer.*kind 5.*QT_8bit"):
        rsxlib.IndexScalarQuantizer(16, qtype, rsxlib.METRIC_INNER_PRODUCT)


def test_sharded_and_refine_forms_are_refused(rsxlib):
    with pytest.raises(RuntimeError, match="IndexScalarQuantizer.*kind 5.*sharded"):
        rsxlib.IndexScalarQuantizer(16, 0, rsxlib.METRIC_L2, devices=[0, 1])
    with pytest.raises(ValueError, match="RFlat"):
        rsxlib.index_factory(64, "SQ8,RFlat")
    with pytest.raises(ValueError, match="RFlat"):
        rsxlib.parse_index_factory(64, "SQ8,RFlat")
    for bad, tok in (("SQ4", "SQ4"), ("SQ8,Flat", "Flat"), ("SQ8x8", "SQ8x8"), ("IVF16,SQ8,RFlat", "RFlat")):
        with pytest.raises(ValueError, match=tok):
            rsxlib.parse_index_factory(64, bad)


def test_factory_strings_parse(rsxlib):
    assert rsxlib.parse_index_factory(768, "SQ8") == {"transforms": [], "d_index": 768, "base": ("SQ",), "refine": False}
    assert rsxlib.parse_index_factory(768, "PCAR64,SQ8") == {"transforms": [("PCAR", 64)], "d_index": 64, "base": ("SQ",), "refine": False}
    assert rsxlib.parse_index_factory(768, "OPQ16_64,SQ8") == {"transforms": [("OPQ", 16, 64)], "d_index": 64, "base": ("SQ",), "refine": False}
    assert rsxlib.parse_index_factory(768, "IVF16,SQ8")["base"] == ("IVFSQ", 16)


def test_faiss_record_is_refused():
    import rsx_faiss_io
    with pytest.raises(RuntimeError, match="IxSQ.*kind 5"):
        rsx_faiss_io.parse_faiss(b"IxSQ" + bytes(64))


# ------------------------------------------------------------------------------------------ 2. the planes and the bound
def test_kprime_of_the_kind():
    assert [sqflat_ref.kprime(k) for k in (1, 10, 100, 500, 1000, 4096)] == [32, 64, 256, 1024, 2048, 8192]
    assert all(sqflat_ref.kprime(k) >= sq_ref.kprime(k) for k in range(1, 4097))


def test_bit_budget():
    """14 bits while (wmax + 64) 128 d stays below 2^31, fewer beyond; never refused for a d the IVF kind takes"""
    assert [sqflat_ref.wmax(d) for d in (1, 64, 768, 1023)] == [16319] * 4
    assert sqflat_ref.wmax(1100) == (2 ** 31 - 1) // (128 * 1100) - 64 == 15188 and sqflat_ref.wmax(2048) == 8127 and sqflat_ref.wmax(65536) == 191
    for d in (1, 100, 1023, 1024, 1032, 1100, 2048, 4096, 65536):
        W = sqflat_ref.wmax(d)
        assert 0 < W <= 127 * 128 + 63 and (W + 64) * 128 * d < 2 ** 31


def test_planes_of_extreme_queries():
    rng = np.random.RandomState(2)
    d = 40
    t = sq_ref.train(rng.randn(300, d).astype(F32))
    q = rng.randn(6, d).astype(F32)
    q[1] = 0                      # no scale to take: all-zero planes, the score is the constant
    q[2] *= F32(1e-30)            # q' in the subnormals
    q[3] *= F32(1e30)
    q[4, 1:] = 0                  # one dimension carries everything: w = +-wmax there
    h, l, inv, qc = sqflat_ref.planes(t, q)
    w = 128 * h.astype(np.int64) + l
    W = sqflat_ref.wmax(d)
    assert np.abs(w).max() <= W and (w[1] == 0).all() and abs(w[4, 0]) == W and (w[4, 1:] == 0).all()
    assert np.isfinite(inv).all() and (inv > 0).all() and np.isfinite(qc).all()
    assert (np.abs(w[[0, 3, 5]]).max(1) == W).all()


@pytest.mark.parametrize("name", sqflat_ref.SETS)
def test_integer_sums_fit_and_the_bound_holds_for_every_pair(name):
    """|128 A_h| and |A| stay below 2^31 (the epilogue forms A in i32), and the scan's fp32 score of EVERY (query, row) lies within eps
    of the exact score, both metrics — the certificate's premise."""
    c = sq_ref.inputs(name)
    t, codes, xhat = sqflat_ref.quantised(name)
    h, l, inv, qc = sqflat_ref.planes(t, c.q32)
    Ah128, A = sqflat_ref.int_sums(h, l, codes)
    print(f"set {name} d {c.d} wmax {sqflat_ref.wmax(c.d)}: max |128 A_h| {np.abs(Ah128).max()}, max |A| {np.abs(A).max()}")
    assert np.abs(Ah128).max() < 2 ** 31 and np.abs(A).max() < 2 ** 31
    x64, q64 = xhat.astype(np.float64), c.q32.astype(np.float64)
    ip = q64 @ x64.T
    n2 = (x64 ** 2).sum(1)
    bias = (F32(-0.5) * n2.astype(F32)).astype(F32)          # (launch_bias_from_norms: the fp32 norm term halved, exactly)
    for metric in (0, 1):
        eps = sqflat_ref.cert_eps(c.d, metric, t, codes, xhat, c.q32)
        sc = sqflat_ref.scan_scores(A, inv, qc, bias if metric == 1 else None).astype(np.float64)
        exact = ip if metric == 0 else ip - 0.5 * n2[None, :]
        err = np.abs(sc - exact)
        spread = exact.max(1) - exact.min(1)
        print(f"set {name} metric {metric}: max error / eps {np.max(err / eps[:, None]):.4f}, eps / score spread {np.min(eps / spread):.2e} .. {np.max(eps / spread):.2e}")
        assert (err <= eps[:, None]).all()


# ------------------------------------------------------------------------------------------ 3. what the GPU tests lean on
def _capped(name, metric, k):
    """the queries the 5 % re-run cap is asserted over: all of B, C, D; in G and H the crowd queries (four queries at a row stored 41
    times: the k-th and the (K' + 1)-th score are EQUAL for k <= 10) are dropped from the capped set"""
    c = sq_ref.inputs(name)
    return ~getattr(c, "is_crowd_q", np.zeros(len(c.q32), bool))


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", sqflat_ref.SETS)
def test_no_query_sits_within_the_bound_of_its_cut(name, metric):
    """From the oracle alone: no capped query has its exact k-th score within 2 eps of its exact (K' + 1)-th, so the 5 % re-run cap of the
    GPU tests is one the reference itself meets; near-tied positions stay under 2 %."""
    c = sq_ref.inputs(name)
    for k in sqflat_ref.ks_all(name):
        risky = sqflat_ref.uncertifiable(name, metric, k)
        cap = _capped(name, metric, k)
        Dk, _ = sqflat_ref.expected(name, metric, k + 1)
        tol = np.abs(Dk[:, :k][np.isfinite(Dk[:, :k])]).max() * 2.0 ** -23
        share = sq_ref.near_tied(Dk, tol)[cap].mean()
        print(f"set {name} metric {metric} k {k}: capped queries within 2 eps {risky[cap].sum()} of {cap.sum()}, the others {risky[~cap].sum()} of {(~cap).sum()}, "
              f"near-tied share {share:.5f}")
        assert risky[cap].sum() == 0 and share <= 0.02
        if name in ("G", "H") and sq_ref.kprime(k) < c.copies:
            assert risky[~cap].all(), "the crowd defeats any certificate"


def test_set_e_crowd_row_for_the_flat_case():
    """Set E's crowd row was chosen for IVF probing; over ALL rows it must still be every crowd query's best match (both metrics) and lie
    below rank K' + 1 of every other query, so that exactly the six crowd queries are re-run."""
    c = sq_ref.inputs("E")
    crowd_rows = np.concatenate([[c.r0], np.arange(c.n - c.copies, c.n)])
    for metric in (0, 1):
        for k in c.ks:
            kp = sq_ref.kprime(k)
            assert c.copies > kp
            Dp, Ip = sqflat_ref.expected("E", metric, kp + 1)
            assert np.isin(Ip[c.is_crowd_q], crowd_rows).all(), "a crowd query's K' + 1 best are all copies of the crowd row"
            assert (Dp[c.is_crowd_q, 0] == Dp[c.is_crowd_q, kp]).all()
            assert not np.isin(Ip[~c.is_crowd_q], crowd_rows).any(), "the crowd stays out of every other query's candidates"
            risky = sqflat_ref.uncertifiable("E", metric, k)
            print(f"set E metric {metric} k {k}: other queries within 2 eps {risky[~c.is_crowd_q].sum()}")
            assert risky[c.is_crowd_q].all() and risky[~c.is_crowd_q].mean() <= 0.05
            # ids inside the crowd: the oracle orders equal scores by position
            assert (np.diff(Ip[c.is_crowd_q][:, :k], axis=1) > 0).all()


def test_overflow_arrangement_of_set_d():
    """GPU test 'overflowing stage rows': D's rows in ascending order of query 0's score.  Every row behind the threshold phase beats that
    query's running threshold — many more than a 256-key row holds; a few queries of its cluster collect more than 256 as well, every
    other query stays far below."""
    c = sq_ref.inputs("D")
    passing = overflow_passing()
    first = 16384
    over, maybe = passing > 320, passing > 200      # (the scan decides on approximate scores: counts near 256 may fall either way)
    print(f"keys behind the threshold phase: query 0 {passing[0]}, queries above 320 keys {over.sum()}, above 200 keys {maybe.sum()}")
    assert passing[0] == c.n - first > 10 * 256 and over[0] and maybe.sum() <= 0.1 * c.nq


def overflow_passing():
    """keys of every query behind the 16384 rows of the threshold phase at k = 10 (K' = 64), from exact scores, in the order below"""
    c = sq_ref.inputs("D")
    _, _, xhat = sqflat_ref.quantised("D")
    s = c.q32.astype(np.float64) @ xhat[overflow_order()].astype(np.float64).T
    first = 16384
    thr = np.sort(s[:, :first], axis=1)[:, -sqflat_ref.kprime(10)]     # the running K'-th score after the phase
    return (s[:, first:] > thr[:, None]).sum(1)


def overflow_order():
    c = sq_ref.inputs("D")
    _, _, xhat = sqflat_ref.quantised("D")
    return np.argsort(c.q32[0].astype(np.float64) @ xhat.astype(np.float64).T, kind="stable")
