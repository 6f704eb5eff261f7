"""CPU: the range_search ABI (version, symbols), the reference cut of tests/range_ref.py against the Tier-0 oracle, the numpy restatement
of the scan threshold on the GPU tests' inputs, and the preconditions those tests rest on (result sizes per radius, the fp32 radii)."""
import os
import re
import subprocess

import numpy as np
import pytest

import range_ref as rr
from conftest import PKG, REPO

F32 = np.float32
NEW = ["rsx_range_search", "rsx_range_result_get", "rsx_range_result_destroy"]


def test_version_and_symbols(rsxlib):
    assert rsxlib.lib().rsx_version() >= 1006
    header = open(os.path.join(REPO, "include", "rsx.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(PKG, "csrc", "librsx.so")], text=True)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in rsxlib.ABI_SYMBOLS, s
        assert re.search(r" T %s\b" % s, exported), s
        assert getattr(rsxlib.lib(), s) is not None
    assert "Index::range_search" in header and "RangeSearchResult" in header
    assert callable(rsxlib.Index.range_search)
    assert "int64" in rsxlib.Index.range_search.__doc__ and "uint64" in rsxlib.Index.range_search.__doc__


def test_refusals_without_a_gpu(rsxlib):
    """the kinds range_search does not serve are refused before any handle is touched"""
    class Fake(rsxlib.IndexIVFPQ):
        def __init__(self):
            self._h, self.d = None, 8
    with pytest.raises(RuntimeError, match="range_search"):
        Fake().range_search(np.zeros((1, 8), F32), 1.0)
    ref = rsxlib.IndexRefineFlat.__new__(rsxlib.IndexRefineFlat)
    with pytest.raises(RuntimeError, match="range_search"):
        ref.range_search(np.zeros((1, 8), F32), 1.0)


@pytest.mark.parametrize("metric", [0, 1])
def test_cut_agrees_with_tier0(orc, metric):
    x, q = rr.flat_inputs()
    x, q = x[:4000].astype(F32), q[:9].astype(F32)
    radius = {0: 97.0, 1: 54.0}[metric]
    lims, D, I = rr.flat_expected_of(q, x, metric, radius)
    D0, I0 = orc.np_flat_search(q, x, len(x), "ip" if metric == 0 else "l2")
    assert lims[0] == 0 and np.all(np.diff(lims) >= 0) and lims[-1] == len(D) == len(I) and lims[-1] > 0
    for i in range(len(q)):
        m = (D0[i] > F32(radius)) if metric == 0 else (D0[i] < F32(radius))
        assert np.array_equal(I[lims[i]:lims[i + 1]], I0[i][m])
        assert np.array_equal(D[lims[i]:lims[i + 1]], D0[i][m])


def test_cut_is_strict_and_skips_padding():
    D = np.array([[5.0, 3.0, 3.0, 1.0, -np.inf]], F32)
    I = np.array([[4, 2, 9, 7, -1]], np.int64)
    lims, Dc, Ic = rr.cut(D, I, 3.0, 0)
    assert lims.tolist() == [0, 1] and Ic.tolist() == [4]
    lims, Dc, Ic = rr.cut(D, I, np.nextafter(F32(3.0), F32(0)), 0)
    assert lims.tolist() == [0, 3] and Ic.tolist() == [4, 2, 9]
    lims, Dc, Ic = rr.cut(D, I, -1e30, 0)
    assert lims.tolist() == [0, 4]
    Dl = np.array([[0.5, 2.0, 2.0, np.inf]], F32)
    lims, Dc, Ic = rr.cut(Dl, np.array([[3, 1, 5, -1]], np.int64), 2.0, 1)
    assert lims.tolist() == [0, 1] and Ic.tolist() == [3]


def test_flat_radii_give_the_intended_result_sizes():
    want = {0: [(0, 2, 0, 5000), (2500, 3500, 4000, 5000), (15000, 25000, 30000, 40000)],
            1: [(0, 1, 0, 1), (2500, 3500, 4000, 5000), (15000, 25000, 55000, 65000)]}
    for metric in (0, 1):
        for radius, (med_lo, med_hi, max_lo, max_hi) in zip(rr.FLAT_RADII[metric], want[metric]):
            c = np.diff(rr.flat_expected(metric, radius)[0])
            assert med_lo <= np.median(c) <= med_hi and max_lo <= c.max() <= max_hi, (metric, radius, np.median(c), c.max())
        assert (np.diff(rr.flat_expected(metric, rr.FLAT_RADII[metric][0])[0]) == 0).sum() > 100       # many empty rows
        assert np.diff(rr.flat_expected(metric, rr.FLAT_RADII[metric][2])[0]).min() > 1024               # every row overflows 1024 keys


def test_ivf_radii_give_the_intended_result_sizes():
    for metric in (0, 1):
        small, large = rr.IVF_RADII[metric]
        c = np.diff(rr.ivf_expected("ivf", metric, 6, small)[0])
        assert 1 <= np.median(c) <= 200, (metric, np.median(c))
        c = np.diff(rr.ivf_expected("ivf", metric, 6, large)[0])
        assert np.median(c) > 1024 and c.max() < 60000, (metric, np.median(c), c.max())


def members_pass(q32, x32, metric, radius, lims, I, rows_of, max_norm2, storage_f16, q_lossy):
    """every member's approximate ranking score, ANY fp32 value within eps of the exact one, is admitted: its lowest possible
    value, rounded down to fp32, is still >= t"""
    t, eps = rr.threshold(q32, radius, metric, max_norm2, storage_f16, q_lossy)
    worst = np.inf
    for i in range(len(q32)):
        ids = I[lims[i]:lims[i + 1]]
        if len(ids) == 0:
            continue
        r = rr.ranking_scores(q32[i], x32[rows_of(ids)], metric) - float(eps[i])
        lo = r.astype(F32)
        lo = np.where(lo.astype(np.float64) > r, np.nextafter(lo, F32(-np.inf)), lo)
        assert np.all(lo >= t[i]), (i, float((lo - t[i]).min()))
        worst = min(worst, float((r - float(t[i])).min()))
    return worst


@pytest.mark.parametrize("metric", [0, 1])
def test_threshold_admits_every_member_flat(metric):
    x, q = rr.flat_inputs()
    x32, q32 = x.astype(F32), q.astype(F32)
    mx = float((x32.astype(np.float64) ** 2).sum(1).max())
    for radius in rr.FLAT_RADII[metric][:2]:
        lims, _, I = rr.flat_expected(metric, radius)
        members_pass(q32, x32, metric, radius, lims, I, lambda ids: ids, mx, True, False)


@pytest.mark.parametrize("metric", [0, 1])
def test_threshold_admits_every_member_ivf_and_fp32(metric):
    c = rr.ivf_inputs()
    mx = float((c.x32.astype(np.float64) ** 2).sum(1).max())
    radius = rr.IVF_RADII[metric][1]
    lims, _, I = rr.ivf_expected("ivf", metric, 6, radius, True)
    members_pass(c.q32, c.x32, metric, radius, lims, I, lambda ids: (ids - 1000003) // 7, mx, True, False)
    # fp32 rows and queries fp16 cannot represent: the larger bound
    x, q, radius = rr.fp32_case(metric)
    lims, _, I = rr.flat_expected_of(q, x, metric, radius)
    mx = float((x.astype(np.float64) ** 2).sum(1).max())
    members_pass(q, x, metric, radius, lims, I, lambda ids: ids, mx, False, True)


def test_threshold_of_special_queries():
    q = np.ones((3, 8), F32)
    q[1, 3] = np.nan
    q[2, 0] = np.inf
    t, _ = rr.threshold(q, 1.0, 0, 4.0)
    assert np.isfinite(t[0]) and t[0] < 1.0 and t[1] == np.inf and t[2] == np.inf
    # the threshold falls as the radius does (inner product) / as it grows (L2)
    assert rr.threshold(q[:1], 0.5, 0, 4.0)[0][0] < t[0]
    assert rr.threshold(q[:1], 2.0, 1, 4.0)[0][0] < rr.threshold(q[:1], 1.0, 1, 4.0)[0][0]


@pytest.mark.parametrize("metric", [0, 1])
def test_fp32_radius_precondition(orc, metric):
    """a radius with no oracle score within 8 ulp exists for the fp32-storage input: the one the GPU test uses"""
    x, q, radius = rr.fp32_case(metric)
    assert not np.array_equal(x, x.astype(np.float16).astype(F32))
    D, I = orc.flat_search(q, x, len(x), metric)
    assert rr.ulp_distance(D, np.full_like(D, radius)).min() > 8
    c = np.diff(rr.cut(D, I, radius, metric)[0])
    assert 100 < np.median(c) < 2000, np.median(c)
