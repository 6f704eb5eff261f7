"""GPU: the reconstruct family (rsx_reconstruct_batch / rsx_make_direct_map) — stored vectors by id on every index kind and
code layout, the two forms of the direct map, staleness across remove_ids / add / reset, the errors, search_and_reconstruct.  Expected
vectors: tests/reconstruct_ref.py (the oracle alone).  Every comparison is bit-equal, on the uint32 view."""
import ctypes

import numpy as np
import pytest

import reconstruct_ref as ref
import util

pytestmark = pytest.mark.gpu
F32 = np.float32
N, NLIST = ref.N, ref.NLIST
_built = {}


def same_bits(got, want, what):
    got, want = np.atleast_2d(ref.bits(got)), np.atleast_2d(ref.bits(want))
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    bad = np.nonzero((got != want).any(axis=-1))
    assert len(bad[0]) == 0, f"{what}: {len(bad[0])} rows differ, first at {[b[0] for b in bad]}"


def queries(d, nq):
    from oracle import oracle as orc
    return orc.synth_queries(d, NLIST, util.SEED_C, util.SEED_X, 0.5, N, util.SEED_Q, 0.1, 0, nq)


def ivfflat(gpu, d=100, ids=None):
    cen, _ = ref.coarse(d)
    ix = gpu.IndexIVFFlat(None, d, NLIST, gpu.METRIC_INNER_PRODUCT)
    ix.set_centroids(cen)
    x = ref.vectors(d)
    if ids is None:
        ix.add(x)
    else:
        ix.add_with_ids(x, ids)
    return ix, x.astype(F32)


def ivfpq(gpu, d, M, layout=None):
    c = ref.pq_case(d, M)
    ix = gpu.IndexIVFPQ(None, d, NLIST, M, 8, gpu.METRIC_INNER_PRODUCT)
    if layout is not None:
        ix.set_param("pq_layout", layout)
    ix.set_centroids(c.cen)
    ix.set_codebooks(c.cb)
    return ix, c


def make(gpu, name):
    """-> (index, expected stored vectors float32 [N, d]); one populated index per case, shared by the tests that do not change it"""
    if name in _built:
        return _built[name]
    if name == "flat16_d768":
        x = ref.vectors(768)
        ix = gpu.IndexFlatIP(768)
        ix.add(x)
        assert ix.storage_dtype == "float16"
        out = ix, x.astype(F32)
    elif name == "flat32_d100":
        x = ref.vectors(100, False)
        ix = gpu.IndexFlatL2(100)
        ix.add(x)
        assert ix.storage_dtype == "float32"
        out = ix, x
    elif name == "ivfflat_d100":
        out = ivfflat(gpu)
    elif name.startswith("ivfpq"):
        d, M, layout = {"ivfpq_64_16_rot": (64, 16, 1), "ivfpq_64_8_granule": (64, 8, None), "ivfpq_128_64_rot": (128, 64, 1),
                        "ivfpq_192_96_sliced": (192, 96, 2), "ivfpq_192_96_rot": (192, 96, 1)}[name]
        ix, c = ivfpq(gpu, d, M, layout)
        assert ix._get("pq_layout") == (layout or 0)
        ix.add(c.x)
        out = ix, c.xhat
    elif name == "pq_256_64_l2":
        c = ref.pq_case(256, 64, flat=True)
        ix = gpu.IndexPQ(256, 64, 8, gpu.METRIC_L2)
        ix.set_codebooks(c.cb)
        ix.add(c.x)
        assert (ref.bits(c.xhat) == 0x80000000).any(), "the case holds a -0 entry"
        out = ix, c.xhat
    elif name.startswith("ivfsq"):
        c = ref.sq_case(100, name.endswith("res"))
        ix = gpu.IndexIVFScalarQuantizer(None, 100, NLIST, gpu.ScalarQuantizer.QT_8bit, gpu.METRIC_L2, c.by_residual)
        ix.set_centroids(c.cen)
        ix.set_sq_trained(c.trained)
        ix.add(c.x)
        out = ix, c.xhat
    elif name == "refine_ivfpq":
        base, c = ivfpq(gpu, 64, 16, 1)
        ix = gpu.IndexRefineFlat(base, 2.0)
        ix.add(c.x)
        out = ix, c.x.astype(F32)       # IndexRefine::reconstruct: refine_index's row
    else:
        raise KeyError(name)
    _built[name] = out
    return out


KINDS = ["flat16_d768", "flat32_d100", "ivfflat_d100", "ivfpq_64_16_rot", "ivfpq_64_8_granule", "ivfpq_128_64_rot", "ivfpq_192_96_sliced",
         "ivfpq_192_96_rot", "pq_256_64_l2", "ivfsq_d100", "ivfsq_d100_res", "refine_ivfpq"]


@pytest.mark.parametrize("name", KINDS)
def test_every_kind_and_layout(gpu, name):
    """every stored id exactly once in shuffled order (any addressing error changes some row), a batch with repeats, batches of 0 and 1,
    reconstruct and reconstruct_n"""
    ix, xhat = make(gpu, name)
    d = xhat.shape[1]
    assert ix.ntotal == N
    rng = np.random.RandomState(11)
    perm = rng.permutation(N).astype(np.int64)
    R = ix.reconstruct_batch(perm)
    assert isinstance(R, np.ndarray) and R.dtype == F32 and R.shape == (N, d)
    same_bits(R, xhat[perm], name)
    rep = rng.randint(0, N, 700).astype(np.int64)
    rep[100:200] = rep[0]
    same_bits(ix.reconstruct_batch(rep), xhat[rep], name + " repeated keys")
    empty = ix.reconstruct_batch(np.empty(0, dtype=np.int64))
    assert empty.shape == (0, d) and empty.dtype == F32
    same_bits(ix.reconstruct_batch(perm[:1]), xhat[perm[:1]], name + " one key")
    one = ix.reconstruct(int(perm[5]))
    assert one.shape == (d,)
    same_bits(one, xhat[perm[5]], name + " reconstruct")
    same_bits(ix.reconstruct_n(517, 300), xhat[517:817], name + " reconstruct_n")


def test_cuda_keys_give_a_cuda_tensor(gpu):
    import torch
    ix, xhat = make(gpu, "ivfpq_192_96_sliced")
    keys = torch.as_tensor(np.random.RandomState(3).permutation(N)[:1111].astype(np.int64)).to("cuda:0")
    R = ix.reconstruct_batch(keys)
    assert R.is_cuda and R.dtype == torch.float32 and tuple(R.shape) == (1111, 192)
    same_bits(R.cpu().numpy(), xhat[keys.cpu().numpy()], "CUDA keys")
    # an output that is not 16-byte aligned takes the 4-byte stores (the library is given a view one float into a buffer)
    ix2, xhat2 = make(gpu, "flat16_d768")
    buf = torch.zeros(1 + 5 * 768, dtype=torch.float32, device="cuda:0")
    k5 = torch.as_tensor(np.array([5, 4000, 17, 17, N - 1], dtype=np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    st = gpu.lib().rsx_reconstruct_batch(ix2._h, ctypes.c_int64(5), ctypes.c_void_p(k5.data_ptr()), 0, ctypes.c_void_p(buf.data_ptr() + 4))
    assert st == 0
    got = buf.cpu().numpy()
    assert got[0] == 0.0
    same_bits(got[1:].reshape(5, 768), xhat2[k5.cpu().numpy()], "unaligned output")


def test_map_forms(gpu):
    """which ids take which map (rsx_get direct_map_type), and that each serves every id"""
    DM = gpu.DirectMap
    rng = np.random.RandomState(23)
    perm = rng.permutation(N).astype(np.int64)
    # sequential ids: Array, built by the first lookup (FAISS would throw without make_direct_map)
    ix, xhat = ivfflat(gpu)
    assert ix.direct_map_type == DM.NoMap
    same_bits(ix.reconstruct_batch(perm), xhat[perm], "sequential")
    assert ix.direct_map_type == DM.Array and ix.get_timing("direct_map_builds") == 1
    same_bits(ix.reconstruct_batch(perm[:10]), xhat[perm[:10]], "sequential, map reused")
    assert ix.get_timing("direct_map_builds") == 1
    # ... and the hash table on request
    ix.set_direct_map_type(DM.Hashtable)
    assert ix.direct_map_type == DM.Hashtable
    same_bits(ix.reconstruct_batch(perm), xhat[perm], "sequential through the hash table")
    # strided ids and ids above 2^32: Hashtable
    for what, ids in (("strided", 7 * np.arange(N, dtype=np.int64) + 1000003), ("above 2^32", (np.int64(1) << 33) + 3 * np.arange(N, dtype=np.int64))):
        ix, xhat = ivfflat(gpu, ids=ids)
        ix.make_direct_map()
        assert ix.direct_map_type == DM.Hashtable, what
        same_bits(ix.reconstruct_batch(ids[perm]), xhat[perm], what)
        with pytest.raises(RuntimeError, match="rsx error -1"):
            ix.reconstruct_batch(np.array([ids[0], ids[1] + 1], dtype=np.int64))
    # a permutation of [0, n) through add_with_ids: Array
    ids = rng.permutation(N).astype(np.int64)
    ix, xhat = ivfflat(gpu, ids=ids)
    ix.make_direct_map()
    assert ix.direct_map_type == DM.Array
    same_bits(ix.reconstruct_batch(ids[perm]), xhat[perm], "permutation")
    # ... also on a Flat handle with explicit ids
    fx = gpu.IndexFlatIP(100)
    fx.add_with_ids(ref.vectors(100), ids)
    same_bits(fx.reconstruct_batch(ids[perm]), xhat[perm], "Flat with explicit ids")
    assert fx.direct_map_type == DM.Array
    # ids in range with one repeat: falls back to Hashtable; the repeated id is its copy in the lowest (list, offset)
    _, assign = ref.coarse(100)
    ids = np.arange(N, dtype=np.int64)
    ids[N - 1] = 10
    ix, xhat = ivfflat(gpu, ids=ids)
    ix.make_direct_map()
    assert ix.direct_map_type == DM.Hashtable
    first = min((10, N - 1), key=lambda v: (assign[v], v))       # one add: in-list order = insertion order
    other = N - 1 if first == 10 else 10
    assert not np.array_equal(xhat[first], xhat[other])
    same_bits(ix.reconstruct(10), xhat[first], "repeated id")
    keys = perm[perm != N - 1]
    want = xhat[keys].copy()
    want[keys == 10] = xhat[first]
    same_bits(ix.reconstruct_batch(keys), want, "ids with one repeat")
    with pytest.raises(RuntimeError, match=str(N - 1)):
        ix.reconstruct(N - 1)
    # a Flat handle of sequential ids needs no map
    fx, _ = make(gpu, "flat16_d768")
    fx.make_direct_map()
    assert fx.direct_map_type == DM.NoMap


@pytest.mark.parametrize("name", ["ivfflat_d100", "ivfpq_192_96_sliced"])
def test_staleness(gpu, name):
    """the map follows remove_ids (rows move), add and reset; IVF-PQ: beside the row-major code copy of a large-k search"""
    if name == "ivfflat_d100":
        ix, xhat = ivfflat(gpu)
        x = ref.vectors(100)
    else:
        ix, c = ivfpq(gpu, 192, 96, 2)
        x, xhat = c.x, c.xhat
        ix.add(x)
        ix.nprobe = 4
        D0, I0 = ix.search(queries(192, 32), 1000)       # K' >= 256: builds the row-major copy of the codes
    rng = np.random.RandomState(31)
    perm = rng.permutation(N).astype(np.int64)
    same_bits(ix.reconstruct_batch(perm), xhat[perm], name)
    if name != "ivfflat_d100":
        D1, I1 = ix.search(queries(192, 32), 1000)
        assert np.array_equal(I0, I1) and np.array_equal(D0, D1), "search beside the map"
    removed = np.arange(3, N, 10, dtype=np.int64)
    kept = np.setdiff1d(np.arange(N, dtype=np.int64), removed)
    assert ix.remove_ids(removed) == len(removed)
    assert ix.direct_map_type == gpu.DirectMap.NoMap, "a mutation releases the map"
    sk = kept[rng.permutation(len(kept))]
    same_bits(ix.reconstruct_batch(sk), xhat[sk], name + " survivors (their rows moved)")
    for key in (removed[0], removed[-1]):
        with pytest.raises(RuntimeError, match=rf"rsx error -1.*key {key} "):
            ix.reconstruct(int(key))
    with pytest.raises(RuntimeError, match=f"key {removed[7]} "):
        ix.reconstruct_batch(np.concatenate([kept[:50], removed[7:9], kept[50:60]]))
    same_bits(ix.reconstruct_batch(sk[:100]), xhat[sk[:100]], name + " after an error")
    ix.add_with_ids(x[removed], removed)
    assert ix.ntotal == N
    same_bits(ix.reconstruct_batch(perm), xhat[perm], name + " after adding the removed vectors back")
    ix.reset()
    with pytest.raises(RuntimeError, match="rsx error -1"):
        ix.reconstruct(0)
    ix.add(x)
    same_bits(ix.reconstruct_batch(perm), xhat[perm], name + " after reset and add")


def test_errors(gpu):
    ix, xhat = make(gpu, "ivfflat_d100")
    L = gpu.lib()
    for keys, named in (([5, N + 5, N + 9], N + 5), ([2, -1, 3], -1), ([N], N)):
        with pytest.raises(RuntimeError, match=rf"rsx error -1.*key {named} ") as e:
            ix.reconstruct_batch(np.array(keys, dtype=np.int64))
        assert "reconstruct_batch" in str(e.value)
        same_bits(ix.reconstruct_batch(np.array([5, 3], dtype=np.int64)), xhat[[5, 3]], "a correct call after the error")
    fx, fhat = make(gpu, "flat16_d768")
    with pytest.raises(RuntimeError, match=rf"rsx error -1.*key {N} "):
        fx.reconstruct(N)
    same_bits(fx.reconstruct(N - 1), fhat[N - 1], "Flat after the error")
    # refused with a message naming the call, the handle untouched: n < 0, a null pointer with n > 0
    out = np.zeros((2, 100), dtype=F32)
    keys = np.array([1, 2], dtype=np.int64)
    kp, op = keys.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    for args in ((ctypes.c_int64(-1), kp, 0, op), (ctypes.c_int64(2), None, 0, op), (ctypes.c_int64(2), kp, 0, None)):
        assert L.rsx_reconstruct_batch(ix._h, *args) == -1
        assert "reconstruct_batch" in L.rsx_last_error().decode()
    assert not out.any()
    assert L.rsx_reconstruct_batch(ix._h, ctypes.c_int64(0), None, 0, None) == 0
    assert L.rsx_make_direct_map(ix._h, 7) == -1 and "make_direct_map" in L.rsx_last_error().decode()
    same_bits(ix.reconstruct_batch(keys), xhat[keys], "after the refusals")


def test_sharded_handle_is_refused(gpu):
    sh = gpu.IndexFlatIP(64, devices=[0, 0])
    assert sh.nshards == 2
    sh.add(ref.vectors(64)[:500])
    for call in (lambda: sh.reconstruct(3), lambda: sh.reconstruct_batch(np.arange(4)), lambda: sh.reconstruct_n(0, 4),
                 lambda: sh.search_and_reconstruct(ref.vectors(64)[:2].copy(), 3)):
        with pytest.raises(RuntimeError, match="rsx error -6: reconstruct_batch.*sharded"):
            call()
    with pytest.raises(RuntimeError, match="rsx error -6: make_direct_map.*sharded"):
        sh.make_direct_map()
    D, I = sh.search(ref.vectors(64)[:2], 3)      # the handle is untouched
    assert sh.ntotal == 500 and I.shape == (2, 3) and (I >= 0).all()


ONES = np.uint32(0xFFFFFFFF)


def check_sar(ix, xhat, q, k, params, what):
    D, I, R = ix.search_and_reconstruct(q, k, params=params)
    D2, I2 = ix.search(q, k, params=params)
    assert np.array_equal(I, I2) and np.array_equal(ref.bits(D), ref.bits(D2)), what + ": D, I are what search returns"
    assert R.shape == (len(q), k, xhat.shape[1]) and R.dtype == F32
    want = xhat[np.where(I >= 0, I, 0)]
    want.view(np.uint32)[I < 0] = ONES
    same_bits(R, want, what)
    return I


def test_search_and_reconstruct(gpu):
    fx, fhat = make(gpu, "flat16_d768")
    check_sar(fx, fhat, queries(768, 9), 10, None, "Flat")
    ix, xhat = make(gpu, "ivfpq_192_96_sliced")
    q = queries(192, 33)
    ix.nprobe = 4
    check_sar(ix, xhat, q, 10, None, "IVF-PQ")
    # nprobe 1 and k larger than the closest list: the -1 positions hold all-ones words
    ix.nprobe = 1
    I = check_sar(ix, xhat, q, 1000, None, "IVF-PQ, nprobe 1")
    assert (I < 0).any() and (I >= 0).any()
    I = check_sar(ix, xhat, q, 1000, gpu.SearchParametersIVF(nprobe=2), "IVF-PQ, nprobe 2 per call")
    ix.nprobe = 4
    sel = gpu.IDSelectorRange(1000, 1400)
    I = check_sar(ix, xhat, q, 100, gpu.SearchParametersIVF(sel=sel, nprobe=NLIST), "IVF-PQ with a selector")
    assert ((I >= 1000) & (I < 1400) | (I < 0)).all() and (I >= 0).any()
    sx, shat = make(gpu, "ivfsq_d100_res")
    sx.nprobe = 4
    check_sar(sx, shat, queries(100, 17).astype(F32), 10, None, "IVF-SQ")
    rx, rhat = make(gpu, "refine_ivfpq")
    rx.base_index.nprobe = 4
    check_sar(rx, rhat, queries(64, 8), 5, None, "IndexRefineFlat")


def test_search_and_reconstruct_cuda_tensors(gpu):
    import torch
    ix, xhat = make(gpu, "ivfpq_64_16_rot")
    ix.nprobe = 1
    q = queries(64, 12)
    D, I, R = ix.search_and_reconstruct(torch.as_tensor(q).to("cuda:0"), 1000)
    assert D.is_cuda and I.is_cuda and R.is_cuda and tuple(R.shape) == (12, 1000, 64)
    Dn, In, Rn = ix.search_and_reconstruct(q, 1000)
    assert isinstance(Rn, np.ndarray)
    assert np.array_equal(I.cpu().numpy(), In) and np.array_equal(ref.bits(D.cpu().numpy()), ref.bits(Dn))
    same_bits(R.cpu().numpy(), Rn, "tensors in, tensors out")
    want = xhat[np.where(In >= 0, In, 0)]
    want.view(np.uint32)[In < 0] = ONES
    assert (In < 0).any()
    same_bits(Rn, want, "IVF-PQ rotated M = 16")


def test_make_direct_map_false_releases_the_map(gpu):
    ix, xhat = ivfflat(gpu)
    keys = np.arange(0, N, 7, dtype=np.int64)
    same_bits(ix.reconstruct_batch(keys), xhat[keys], "first")
    w0 = ix._get("workspace_bytes")
    assert ix.direct_map_type == gpu.DirectMap.Array
    ix.make_direct_map(False)
    w1 = ix._get("workspace_bytes")
    assert ix.direct_map_type == gpu.DirectMap.NoMap and w0 - w1 == 8 * N, (w0, w1)     # Array: 8 B per vector
    same_bits(ix.reconstruct_batch(keys), xhat[keys], "the next lookup rebuilds the map")
    assert ix.direct_map_type == gpu.DirectMap.Array and ix.get_timing("direct_map_builds") == 2
    ix.set_direct_map_type(gpu.DirectMap.Hashtable)
    assert ix._get("workspace_bytes") - w1 == 16 * 16384      # 16 B per slot, the power of two >= 2 N slots
    ix.set_direct_map_type(gpu.DirectMap.NoMap)
    assert ix._get("workspace_bytes") == w1
