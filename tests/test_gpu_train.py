"""GPU: rsx_train against the oracle's training, bit for bit, at the shapes the index runs at.

Every search test either injects the oracle's centroids / codebooks or reads the GPU's back and hands them to the oracle, so a
training bug at a product shape would leave them all green.  Here each case restates the product's pipeline with oracle functions
(FAISS Clustering::train / ProductQuantizer::train) and requires the same bits:

  coarse:  kmeans_sample(n, nlist, 256, 1234) -> kmeans(0, ..., 10, 1234)
  PQ:      kmeans_sample(n, 256, 256, 1234) -> assign_ip -> residuals -> pq_train(..., 25, 1234)

The shapes reach what test_gpu_ivf.py::test_train_matches_oracle (d 64, M 8, nlist 8) does not: several arg-max column tiles of 128
centroids with a ragged last one, both subsamples, every k_pq_encode specialisation, degenerate data that reaches the empty-cluster
split and the tie rules, every input form, sharded handles, and one end-to-end search in which no GPU-trained parameter reaches the
oracle."""
import numpy as np
import pytest

from util import SEED_C, SEED_X, SEED_Q, assert_same_results

pytestmark = pytest.mark.gpu

SEED = 1234          # the product's training seed (api_build.hip train_impl)
_cache = {}


def oracle_train(orc, x32, nlist, M=None):
    """(centroids, codebooks or None): the product's training pipeline restated with oracle functions."""
    n = x32.shape[0]
    cen = orc.kmeans(0, x32[orc.kmeans_sample(n, nlist, 256, SEED)], nlist, 10, SEED)
    if M is None:
        return cen, None
    sel = orc.kmeans_sample(n, 256, 256, SEED)
    a, _ = orc.assign_ip(cen, x32[sel])
    return cen, orc.pq_train(orc.residuals(cen, x32[sel], a), M, 25, SEED)


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def make(gpu, kind, d, nlist, M=None, metric=0, devices=None):
    if kind == "ivfflat":
        return gpu.IndexIVFFlat(None, d, nlist, metric, devices=devices)
    return gpu.IndexIVFPQ(None, d, nlist, M, 8, metric, devices=devices)


def assert_equal(got, want, what):
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    assert np.isfinite(want).all(), f"{what}: the oracle's parameters are not finite"
    if not np.array_equal(got, want):
        rows = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(rows)} of {got.shape[0]} rows differ (first {rows[:6].tolist()}), "
                             f"max abs diff {np.abs(got - want).max()}")


def check_trained(ix, cen, cb, what):
    assert ix.is_trained, what
    assert_equal(ix.get_centroids(), cen, f"{what}: centroids")
    if cb is not None:
        assert_equal(ix.get_codebooks(), cb, f"{what}: codebooks")


def synth(orc, d, n, ncent=64, seed_x=SEED_X):
    return orc.synth_vectors(d, ncent, SEED_C, seed_x, 0.5, 0, n)


def initial_codebooks(orc, res, M):
    """The codewords PQ training starts from (orc_pq_train: k-means per sub-space with seed + m, niter 0 = initialisation)."""
    dsub = res.shape[1] // M
    return np.stack([orc.kmeans(1, res[:, m * dsub:(m + 1) * dsub], 256, 0, SEED + m) for m in range(M)])


# ---------------------------------------------------------------- 1. coarse quantiser at real tile shapes
# nlist 160 / 300 / 1000 / 4096: 2 / 3 / 8 / 32 arg-max column tiles, the last one holding 32 / 44 / 104 / 128 centroids.
TILE_CASES = [
    # kind,      d,   nlist, M,    n,               metric
    ("ivfflat", 768, 160, None, 256 * 160, 0),            # n = 256 nlist: no subsample
    ("ivfflat", 768, 160, None, 256 * 160, 1),            # METRIC_L2: still spherical IP k-means (pinned)
    ("ivfflat", 768, 300, None, 256 * 300 + 4321, 0),     # coarse subsample
    ("ivfpq", 768, 160, 16, 256 * 160 + 2000, 0),         # both subsamples, dsub 48
    ("ivfpq", 100, 1000, 25, 256 * 1000, 0),              # eight tiles, no coarse subsample, PQ subsample, dsub 4
    ("ivfpq", 100, 300, 10, 256 * 300 + 999, 0),          # both subsamples, generic k_pq_encode (dsub 10)
    ("ivfflat", 100, 1000, None, 256 * 1000 + 777, 0),    # eight tiles, subsample
    ("ivfpq", 768, 4096, 96, 6 * 4096, 0),                # the headline nlist and M: 32 tiles, six points per centroid
]


@pytest.mark.parametrize("kind,d,nlist,M,n,metric", TILE_CASES,
                         ids=[f"{c[0]}-d{c[1]}-nlist{c[2]}-M{c[3]}-n{c[4]}-metric{c[5]}" for c in TILE_CASES])
def test_train_tiles(gpu, orc, kind, d, nlist, M, n, metric):
    x = synth(orc, d, n)
    cen, cb = cached(("tiles", d, nlist, M, n), lambda: oracle_train(orc, x.astype(np.float32), nlist, M))
    ix = make(gpu, kind, d, nlist, M, metric)
    ix.train(x)
    check_trained(ix, cen, cb, f"{kind} d {d} nlist {nlist} M {M} n {n} metric {metric}")


# ---------------------------------------------------------------- 2. input forms, 6. sharded handles and repeated training
FORM_SHAPE = dict(d=128, nlist=200, M=16, n=20000)


def form_data(orc):
    def build():
        s = FORM_SHAPE
        x16 = synth(orc, s["d"], s["n"])
        rng = np.random.RandomState(3)
        x32 = x16.astype(np.float32) + rng.uniform(-1e-3, 1e-3, x16.shape).astype(np.float32)
        assert (x32.astype(np.float16).astype(np.float32) != x32).mean() > 0.99, "the fp32 input must not be fp16 values"
        return x16, x32, oracle_train(orc, x16.astype(np.float32), s["nlist"], s["M"]), oracle_train(orc, x32, s["nlist"], s["M"])
    return cached("forms", build)


@pytest.mark.parametrize("form", ["f16_numpy", "f32_numpy", "f16_torch_cuda", "f32_torch_cuda"])
def test_train_input_forms(gpu, orc, form):
    import torch
    s = FORM_SHAPE
    x16, x32, (cen16, cb16), (cen32, cb32) = form_data(orc)
    src, cen, cb = (x16, cen16, cb16) if form.startswith("f16") else (x32, cen32, cb32)
    if form.endswith("torch_cuda"):
        src = torch.from_numpy(src).cuda()
    ix = make(gpu, "ivfpq", s["d"], s["nlist"], s["M"])
    ix.train(src)
    check_trained(ix, cen, cb, form)
    flat = make(gpu, "ivfflat", s["d"], s["nlist"])
    flat.train(src)
    check_trained(flat, cen, None, f"{form} (IVF-Flat)")


def test_train_sharded_equals_single_and_oracle(gpu, orc):
    s = FORM_SHAPE
    x16, _, (cen, cb), _ = form_data(orc)
    single = make(gpu, "ivfpq", s["d"], s["nlist"], s["M"])
    single.train(x16)
    sh = make(gpu, "ivfpq", s["d"], s["nlist"], s["M"], devices=[0, 0])
    assert sh.nshards == 2
    sh.train(x16)
    check_trained(sh, cen, cb, "sharded")
    check_trained(single, sh.get_centroids(), sh.get_codebooks(), "single vs sharded")
    shf = make(gpu, "ivfflat", s["d"], s["nlist"], devices=[0, 0])
    shf.train(x16)
    check_trained(shf, cen, None, "sharded IVF-Flat")


def test_train_twice_same_bits(gpu, orc):
    s = FORM_SHAPE
    x16, _, (cen, cb), _ = form_data(orc)
    ix = make(gpu, "ivfpq", s["d"], s["nlist"], s["M"])
    ix.train(x16)
    c1, b1 = ix.get_centroids(), ix.get_codebooks()
    ix.train(x16)
    check_trained(ix, c1, b1, "second training on the same handle")
    check_trained(ix, cen, cb, "second training vs the oracle")
    other = make(gpu, "ivfpq", s["d"], s["nlist"], s["M"])
    other.train(x16)
    check_trained(other, c1, b1, "a second handle")


def test_train_retrains_given_centroids(gpu, orc):
    """rsx_train always retrains the coarse quantiser, even when it already holds nlist centroids (pinned)."""
    s = FORM_SHAPE
    x16, _, (cen, cb), _ = form_data(orc)
    rng = np.random.RandomState(5)
    ix = make(gpu, "ivfpq", s["d"], s["nlist"], s["M"])
    ix.set_centroids(rng.standard_normal((s["nlist"], s["d"])).astype(np.float32))
    ix.train(x16)
    check_trained(ix, cen, cb, "train after set_centroids")


def test_train_errors_leave_handle_usable(gpu, orc):
    d, nlist, M, n = 32, 8, 8, 3000
    x = synth(orc, d, n, ncent=8)
    for kind in ("ivfflat", "ivfpq"):
        ix = make(gpu, kind, d, nlist, M)
        with pytest.raises(RuntimeError, match="rsx error"):
            ix.train(x[:nlist - 1])                         # fewer points than centroids
        assert not ix.is_trained
        if kind == "ivfpq":
            with pytest.raises(RuntimeError, match="rsx error"):
                ix.train(x[:255])                           # enough for the coarse quantiser, too few for 256 codewords
            assert not ix.is_trained
        ix.train(x)
        cen, cb = oracle_train(orc, x.astype(np.float32), nlist, M if kind == "ivfpq" else None)
        check_trained(ix, cen, cb, f"{kind} after failed trainings")
        # a failed training of a trained handle leaves its parameters as they were
        for bad in ([x[1000:1000 + nlist - 1]] + ([x[1000:1255]] if kind == "ivfpq" else [])):
            with pytest.raises(RuntimeError, match="rsx error"):
                ix.train(bad)
            check_trained(ix, cen, cb, f"{kind} after a failed retraining on {len(bad)} points")
        ix.add(x)
        assert ix.ntotal == n
        a, _ = orc.assign_ip(cen, x.astype(np.float32))
        assert np.array_equal(ix.assign(x), a), f"{kind}: assignment after failed trainings"


# ---------------------------------------------------------------- 3. degenerate data: split path and tie rules
def test_train_repeated_rows(gpu, orc):
    """Forty distinct rows repeated: duplicate initial centroids, exact arg-max ties across column tiles, empty clusters (coarse
    and PQ), so FAISS's split runs in every iteration."""
    d, nlist, M, n = 64, 200, 8, 256 * 200
    rng = np.random.RandomState(7)
    x = synth(orc, d, 40, ncent=8)[rng.randint(0, 40, size=n)]
    x32 = x.astype(np.float32)
    c0 = orc.kmeans(0, x32, nlist, 0, SEED)                  # niter 0: the initial centroids
    first, later = {}, []                                  # later: centroids equal to an earlier one
    for j, r in enumerate(c0):
        i = first.setdefault(r.tobytes(), j)
        if i != j:
            later.append((i, j))
    assert any(i < 128 <= j for i, j in later), "no duplicate initial centroids across the arg-max column tiles"
    a0, _ = orc.assign_ip(c0, x32)
    assert (np.bincount(a0, minlength=nlist) == 0).any(), "no empty cluster after the first assignment"
    assert not np.isin(a0, [j for _, j in later]).any(), "exact ties must go to the first maximum"
    cen, cb = oracle_train(orc, x32, nlist, M)
    a, _ = orc.assign_ip(cen, x32)
    res = orc.residuals(cen, x32, a)
    codes = orc.pq_encode(initial_codebooks(orc, res, M), res)
    assert any((np.bincount(codes[:, m], minlength=256) == 0).any() for m in range(M)), "no empty PQ cluster"
    ix = make(gpu, "ivfpq", d, nlist, M)
    ix.train(x)
    check_trained(ix, cen, cb, "repeated rows")


def test_train_zero_rows(gpu, orc):
    """Zero rows tie at score 0 with every centroid and all go to centroid 0; with positive data and a zero row as initial centroid 0,
    that centroid stays the zero vector, whose renormalisation must be skipped."""
    d, nlist, M, n = 32, 150, 8, 256 * 150
    x32 = np.abs(synth(orc, d, n, ncent=16).astype(np.float32)) + np.float32(0.25)
    probe = np.zeros((n, d), np.float32)
    probe[:, 0] = np.arange(n)
    init_rows = orc.kmeans(1, probe, nlist, 0, SEED)[:, 0].astype(np.int64)   # the rows the initial centroids copy
    x32[::5] = 0.0
    x32[init_rows[0]] = 0.0
    x = x32.astype(np.float16)
    x32 = x.astype(np.float32)
    c0 = orc.kmeans(0, x32, nlist, 0, SEED)
    assert not c0[0].any() and (~c0.any(axis=1)).sum() > 1, "initial centroid 0 (and another) must be zero"
    cen, cb = oracle_train(orc, x32, nlist, M)
    assert not cen[0].any(), "centroid 0 must end as the zero vector"
    ix = make(gpu, "ivfpq", d, nlist, M)
    ix.train(x)
    check_trained(ix, cen, cb, "zero rows")


def test_train_pq_ties_dsub2(gpu, orc):
    """fp16 data on a five-value grid, dsub 2: at most 25 sub-vectors per coarse cluster, so the 256 initial codewords repeat
    (first-minimum ties in k_pq_encode) and PQ clusters are empty."""
    d, nlist, M, n = 16, 4, 8, 6000
    rng = np.random.RandomState(11)
    x = (rng.randint(-2, 3, size=(n, d)) * 0.5).astype(np.float16)
    x32 = x.astype(np.float32)
    cen, cb = oracle_train(orc, x32, nlist, M)
    a, _ = orc.assign_ip(cen, x32)
    res = orc.residuals(cen, x32, a)
    cb0 = initial_codebooks(orc, res, M)
    assert all(len(np.unique(cb0[m], axis=0)) < 256 for m in range(M)), "duplicate initial codewords expected in every sub-space"
    codes = orc.pq_encode(cb0, res)
    assert all((np.bincount(codes[:, m], minlength=256) == 0).any() for m in range(M)), "empty PQ clusters expected"
    ix = make(gpu, "ivfpq", d, nlist, M)
    ix.train(x)
    check_trained(ix, cen, cb, "fp16 grid, dsub 2")


# ---------------------------------------------------------------- 4. PQ codebooks at every k_pq_encode specialisation
# 6, 96, 160: the generic kernel (dsub 10 runs in test_train_tiles); 96: its codebook above 48 KiB of LDS, 160: all 160 KiB
DSUBS = [2, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 160]


@pytest.mark.parametrize("dsub", DSUBS)
def test_train_pq_dsub(gpu, orc, dsub):
    d, nlist, n = (192 if 192 % dsub == 0 else dsub), 40, 5000
    M = d // dsub
    x = synth(orc, d, n, ncent=16)
    cen, cb = cached(("dsub", dsub), lambda: oracle_train(orc, x.astype(np.float32), nlist, M))
    ix = make(gpu, "ivfpq", d, nlist, M)
    ix.train(x)
    check_trained(ix, cen, cb, f"dsub {dsub} (M {M})")


@pytest.mark.parametrize("d,M", [(161, 1), (768, 4)])
def test_pq_dsub_beyond_lds_is_refused(gpu, d, M):
    """256 codewords of d / M > 160 floats do not fit k_pq_encode's 160 KiB of LDS (dsub 160 trains in test_train_pq_dsub): such an
    index is refused at creation.  At dsub 192 the encode launch used to be rejected silently, so training built codebooks from codes
    that were never written and the launch error surfaced in the next search."""
    with pytest.raises(RuntimeError, match="rsx error"):
        make(gpu, "ivfpq", d, 40, M)


D768 = dict(d=768, nlist=300, n=20000, nq=64)


def d768_data(orc, M):
    s = D768

    def build_x():
        x = synth(orc, s["d"], s["n"])
        q = orc.synth_queries(s["d"], 64, SEED_C, SEED_X, 0.5, s["n"], SEED_Q, 0.1, 0, s["nq"])
        return x, q
    x, q = cached("d768", build_x)
    cen, cb = cached(("d768", M), lambda: oracle_train(orc, x.astype(np.float32), s["nlist"], M))
    return x, q, cen, cb


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_train_m96_every_layout(gpu, orc, layout):
    s = D768
    x, _, cen, cb = d768_data(orc, 96)
    ix = make(gpu, "ivfpq", s["d"], s["nlist"], 96)
    ix.set_param("pq_layout", layout)
    assert ix._get("pq_layout") == layout
    ix.train(x)
    check_trained(ix, cen, cb, f"M 96 pq_layout {layout}")


def test_train_m16_d768(gpu, orc):
    s = D768
    x, _, cen, cb = d768_data(orc, 16)
    ix = make(gpu, "ivfpq", s["d"], s["nlist"], 16)
    ix.train(x)
    check_trained(ix, cen, cb, "M 16 at d 768")


# ---------------------------------------------------------------- 5. PQ subsample at a small d
def test_train_pq_subsample(gpu, orc):
    d, nlist, M, n = 32, 64, 16, 70000            # coarse keeps 16384 of 70000, PQ keeps 65536
    x = synth(orc, d, n, ncent=32)
    cen, cb = oracle_train(orc, x.astype(np.float32), nlist, M)
    ix = make(gpu, "ivfpq", d, nlist, M)
    ix.train(x)
    check_trained(ix, cen, cb, "PQ subsample")


# ---------------------------------------------------------------- 7. end to end with oracle-only parameters
def test_train_add_search_all_oracle(gpu, orc):
    """GPU train + add + search against the oracle's train -> assign -> residuals -> encode -> scan from the same raw vectors."""
    s, M, nprobe = D768, 96, 16
    x, q, cen, cb = d768_data(orc, M)
    x32 = x.astype(np.float32)
    ix = make(gpu, "ivfpq", s["d"], s["nlist"], M)
    ix.train(x)
    ix.add(x)
    ix.nprobe = nprobe
    a, _ = orc.assign_ip(cen, x32)
    lm = orc.ListMajor(a, np.arange(s["n"]), orc.pq_encode(cb, orc.residuals(cen, x32, a)), s["nlist"])
    for k in (10, 100):
        D, I = ix.search(q, k)
        Dr, Ir = orc.ivfpq_search(cen, cb, lm, q.astype(np.float32), nprobe, k)
        assert_same_results(D, I, Dr, Ir, f"train + add + search, k {k}")
