"""CPU: the QT_8bit scalar quantiser's numpy restatement (tests/sq_ref.py), the Python surface and ABI of IndexIVFScalarQuantizer, and the
preconditions the GPU tests (tests/test_gpu_sq.py) lean on, asserted from the oracle alone."""
import os
import re

import numpy as np
import pytest

import sq_ref
import util
from conftest import REPO

F32 = np.float32
SETS = ["A", "B", "C", "D"]


# ------------------------------------------------------------------------------------------ the helper itself
def _data(seed=3, n=500, d=24):
    rng = np.random.RandomState(seed)
    return (rng.randn(n, d) * rng.uniform(0.01, 3.0, d) + rng.uniform(-2, 2, d)).astype(F32)


def test_decode_encode_is_idempotent_on_codes():
    y = _data()
    t = sq_ref.train(y)
    codes = np.random.RandomState(1).randint(0, 256, (2000, y.shape[1])).astype(np.uint8)
    assert np.array_equal(sq_ref.encode(t, sq_ref.decode(t, codes)), codes)
    c2 = sq_ref.encode(t, y)
    assert np.array_equal(sq_ref.encode(t, sq_ref.decode(t, c2)), c2)


def test_reconstruction_error_inside_the_trained_range():
    y = _data(4)
    t = sq_ref.train(y)
    d = y.shape[1]
    r = sq_ref.decode(t, sq_ref.encode(t, y))
    assert (np.abs(r.astype(np.float64) - y) <= t[d:].astype(np.float64) / 510 * (1 + 1e-4)).all()
    codes = sq_ref.encode(t, y)
    assert codes.min() == 0 and codes.max() == 255      # the extremes of every dimension are trained values


def test_constant_dimension_and_clamping():
    y = _data(5)
    y[:, 2] = F32(0.75)
    t = sq_ref.train(y)
    d = y.shape[1]
    assert t[d + 2] == 0 and t[2] == F32(0.75)
    codes = sq_ref.encode(t, y)
    assert (codes[:, 2] == 0).all()
    assert (sq_ref.decode(t, codes)[:, 2] == F32(0.75)).all()
    lo = (t[:d] - F32(1.0))[None, :].astype(F32)
    hi = (t[:d] + t[d:] + F32(1.0))[None, :].astype(F32)
    keep = np.arange(d) != 2
    assert (sq_ref.encode(t, lo)[0, keep] == 0).all() and (sq_ref.encode(t, hi)[0, keep] == 255).all()
    assert sq_ref.encode(t, hi)[0, 2] == 0              # vdiff == 0: code 0 whatever the value


def test_train_is_min_and_range_in_fp32():
    y = _data(6)
    t = sq_ref.train(y)
    d = y.shape[1]
    assert t.dtype == F32 and t.shape == (2 * d,)
    assert np.array_equal(t[:d], y.min(0)) and np.array_equal(t[d:], (y.max(0) - y.min(0)).astype(F32))


@pytest.mark.parametrize("by_residual", [False, True])
@pytest.mark.parametrize("metric", [0, 1])
def test_probing_every_list_equals_the_flat_oracle_over_the_stored_vectors(orc, metric, by_residual):
    c = sq_ref.inputs("C")
    assert c.nprobe == c.nlist
    _, _, xhat = sq_ref.quantised("C", by_residual)
    D, I = sq_ref.expected("C", metric, by_residual, 100)
    Dr, Ir = orc.flat_search(c.q32, xhat, 100, metric)
    util.assert_same_results(D, I, Dr, Ir, "IVF oracle over every list vs Flat oracle")


# ------------------------------------------------------------------------------------------ Python surface and ABI
def test_scalar_quantizer_constants(rsxlib):
    SQ = rsxlib.ScalarQuantizer
    assert (SQ.QT_8bit, SQ.QT_4bit, SQ.QT_8bit_uniform, SQ.QT_4bit_uniform, SQ.QT_fp16, SQ.QT_8bit_direct, SQ.QT_6bit) == (0, 1, 2, 3, 4, 5, 6)


def test_abi_version_and_kind(rsxlib):
    assert rsxlib.lib().rsx_version() >= 1005
    header = open(os.path.join(REPO, "include", "rsx.h")).read()
    assert re.search(r"RSX_KIND_IVFSQ\s*=\s*4", header)
    for s in ("rsx_ivfsq_create", "rsx_set_sq_trained", "rsx_get_sq_trained"):
        assert s in rsxlib.ABI_SYMBOLS and getattr(rsxlib.lib(), s) is not None


def test_no_cpu_path(rsxlib):
    if rsxlib.get_num_gpus() > 0:
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        rsxlib.IndexIVFScalarQuantizer(None, 16, 4, rsxlib.ScalarQuantizer.QT_8bit, rsxlib.METRIC_INNER_PRODUCT)


@pytest.mark.parametrize("qtype", [1, 2, 3, 4, 5, 6])
def test_other_qtypes_are_refused(rsxlib, qtype):
    with pytest.raises(RuntimeError, match="QT_8bit.*IndexIVFFlat"):
        rsxlib.IndexIVFScalarQuantizer(None, 16, 4, qtype, rsxlib.METRIC_INNER_PRODUCT)


def test_l2_coarse_quantiser_is_refused(rsxlib):
    class Q:
        metric_type = rsxlib.METRIC_L2
    with pytest.raises(RuntimeError, match="inner-product coarse"):
        rsxlib.IndexIVFScalarQuantizer(Q(), 16, 4, 0, rsxlib.METRIC_L2)


def test_faiss_record_is_refused():
    import rsx_faiss_io
    with pytest.raises(RuntimeError, match="IwSq.*kind 4"):
        rsx_faiss_io.parse_faiss(b"IwSq" + bytes(64))


# ------------------------------------------------------------------------------------------ preconditions of the GPU tests
def test_list_lengths_cover_the_work_item_sizes():
    """(A) most lists shorter than one 512-row work item, one of fewer than 16 rows; (B) lists on both sides of 512 rows, 70 queries fill no
    group; (C) padded rows, every list probed; (D) lists of more than one 1024-row work item, and query counts on both sides of the
    threshold between the 16-query and the 64-query form."""
    a, b, c, d = (sq_ref.inputs(s) for s in SETS)
    for s in (a, b, c, d):
        print(f"set {s.name}: list sizes {s.sizes.min()} .. {s.sizes.max()}")
    assert np.median(a.sizes) < 512 and 0 < a.sizes.min() < 16
    assert b.sizes.min() < 512 < b.sizes.max() and b.nq % 16 != 0 and b.nq > 64
    assert c.d % 64 != 0 and c.nprobe == c.nlist
    assert d.sizes.max() > 1024 and d.nq * d.nprobe // d.nlist >= 48 and 20 * d.nprobe // d.nlist < 12


def _kprime(k):
    return k + max(8, k // 16)      # the first re-score depth (api_search.hip: finalize_args)


@pytest.mark.parametrize("by_residual", [False, True])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", SETS)
def test_near_ties_and_certificate_gaps(name, metric, by_residual):
    """Near-ties: positions (rank k + 1 included) whose oracle score lies within 2 tol of a neighbour's stay under 2 % per input set.
    Certificate: queries whose gap between the exact k-th and the exact (K' + 1)-th score is under twice the bound the kernel uses stay
    under the 5 % re-run cap."""
    c = sq_ref.inputs(name)
    t, codes, xhat = sq_ref.quantised(name, by_residual)
    for k in c.ks:
        Dk, _ = sq_ref.expected(name, metric, by_residual, k + 1)
        tol = np.abs(Dk[:, :k][np.isfinite(Dk[:, :k])]).max() * 2.0 ** -23      # the GPU tests' tolerance: from the k results
        share = sq_ref.near_tied(Dk, tol).mean()
        print(f"set {name} metric {metric} by_residual {by_residual} k {k}: near-tied share {share:.5f}")
        assert share <= 0.02
        kp = _kprime(k)
        Dp, _ = sq_ref.expected(name, metric, by_residual, kp + 1)
        eps = sq_ref.cert_eps(c.d, metric, by_residual, t, c.cen, codes, xhat, c.q32)
        if metric == 1:      # the scan ranks by <q, x> - |x|^2 / 2: a distance moves by twice the bound, plus the conversion's roundings
            q2 = (c.q32.astype(np.float64) ** 2).sum(1)
            eps = 2 * eps + 3e-7 * (2 * np.abs(Dp[:, kp].astype(np.float64)) + 2 * q2)
        gap = np.abs(Dp[:, kp].astype(np.float64) - Dp[:, k - 1])
        risky = np.isfinite(Dp[:, kp]) & (gap < 2 * eps)
        print(f"set {name} metric {metric} by_residual {by_residual} k {k}: eps max {np.max(eps):.3e}, queries within 2 eps {risky.mean():.5f}")
        assert risky.mean() <= 0.05
