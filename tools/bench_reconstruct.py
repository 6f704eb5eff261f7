#!/usr/bin/env python3
"""Reconstruct measurement: on the headline 100M x 768 IVF-PQ index (nlist 4096, M 96, sliced layout) and on a 10M x 768
Flat index (fewer vectors when the free device memory does not hold them: the size is printed) —
  * the direct map's build, Array and Hashtable (a Flat index of sequential ids needs none);
  * reconstruct_batch of 1024 x 10 and 1024 x 1000 random stored ids, CUDA tensors in and out: ms per call and output bytes per second
    beside the HBM rate a streaming kernel reaches on an MI355X (6.3 TB/s);
  * search_and_reconstruct beside search at k = 10 and k = 1000, ms per 1024-query batch;
and, for scale, the only route there was before on a 1M x 768 IVF-PQ index: get_list of every list, then host indexing and decoding.
One JSON line per case on stdout; --out writes the table as markdown.

  python tools/bench_reconstruct.py [--n-pq 100000000] [--n-flat 10000000] [--n-old 1000000] [--steps 3] [--out profiles/reconstruct_speed.md]
"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retrieval-scaling_amd")); sys.path.insert(0, REPO)
import numpy as np

D, NC, SC, SX, SQ = 768, 4096, 1234, 10000, 999
HBM_TBS = 6.3
ROWS = []


def emit(**kw):
    ROWS.append(kw)
    print(json.dumps(kw), flush=True)


def fill(rsx, torch, ix, n):
    buf = torch.empty((1_000_000, D), dtype=torch.float16, device="cuda:0")
    for c0 in range(0, n, 1_000_000):
        nb = min(1_000_000, n - c0)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, c0, nb, out=buf[:nb])
        ix.add(buf[:nb])
    del buf


def train_ivfpq(rsx, torch, n, nlist, M):
    ix = rsx.IndexIVFPQ(rsx.IndexFlatIP(D), D, nlist, M, 8, rsx.METRIC_INNER_PRODUCT, device=0)
    nt = min(n, 256 * nlist)
    xt = torch.empty((nt, D), dtype=torch.float16, device="cuda:0")
    stride = max(1, n // nt)
    for b in range(0, nt, 4096):
        nb = min(4096, nt - b)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, (b * stride) % max(1, n - nb), nb, out=xt[b:b + nb])
    ix.train(xt)
    del xt
    return ix


def ms_of(torch, fn, steps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def measure(rsx, torch, ix, name, n, args, with_map):
    rng = np.random.default_rng(5)
    if with_map:
        for form, typ in (("Array", rsx.DirectMap.Array), ("Hashtable", rsx.DirectMap.Hashtable)):
            ix.set_direct_map_type(rsx.DirectMap.NoMap)
            w0 = ix._get("workspace_bytes")
            t0 = time.perf_counter(); ix.set_direct_map_type(typ); ms = (time.perf_counter() - t0) * 1e3
            assert ix.direct_map_type == typ
            emit(index=name, case=f"direct map build, {form}", ms=round(ms, 2), map_bytes_per_vector=round((ix._get("workspace_bytes") - w0) / n, 1))
        ix.set_direct_map_type(rsx.DirectMap.NoMap)
        ix.set_direct_map_type(rsx.DirectMap.Array)      # the map the lookups below use
    else:
        emit(index=name, case="direct map build", ms=None, note="sequential ids: the key is the row, no map")
    for per in (10, 1000):
        keys = torch.as_tensor(rng.integers(0, n, args.batch * per)).to("cuda:0")
        ms = ms_of(torch, lambda: ix.reconstruct_batch(keys), args.steps)
        tbs = keys.numel() * D * 4 / (ms * 1e-3) / 1e12
        emit(index=name, case=f"reconstruct_batch {args.batch} x {per} keys", ms=round(ms, 3), out_TB_per_s=round(tbs, 3), of_hbm=round(tbs / HBM_TBS, 3))
        del keys
    Q = torch.empty((args.batch, D), dtype=torch.float16, device="cuda:0")
    rsx.synth_queries(D, NC, SC, SX, 0.5, n, SQ, 0.1, 0, args.batch, out=Q)
    for k in (10, 1000):
        ms_s = ms_of(torch, lambda: ix.search(Q, k), args.steps)
        ms_r = ms_of(torch, lambda: ix.search_and_reconstruct(Q, k), args.steps)
        emit(index=name, case=f"search_and_reconstruct k={k}", ms=round(ms_r, 3), search_ms=round(ms_s, 3), gather_ms=round(ms_r - ms_s, 3))


def old_route(rsx, torch, args):
    """what a caller had to do before: download every list, index and decode on the host"""
    n, nlist, M = args.n_old, 1024, 96
    ix = train_ivfpq(rsx, torch, n, nlist, M)
    fill(rsx, torch, ix, n)
    keys = np.random.default_rng(5).integers(0, n, args.batch * 10)
    t0 = time.perf_counter()
    cb, cen = ix.get_codebooks(), ix.get_centroids()
    codes, ids, lists = [], [], []
    for l in range(nlist):
        c, i = ix.get_list(l)
        codes.append(c); ids.append(i); lists.append(np.full(len(i), l, dtype=np.int32))
    codes, ids, lists = np.concatenate(codes), np.concatenate(ids), np.concatenate(lists)
    order = np.argsort(ids)
    pos = order[np.searchsorted(ids[order], keys)]
    dsub = D // M
    old = cen[lists[pos]].copy()
    for m in range(M):
        old[:, m * dsub:(m + 1) * dsub] += cb[m][codes[pos, m]]
    ms_old = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter(); new = ix.reconstruct_batch(keys); ms_first = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter(); ix.reconstruct_batch(keys); ms_next = (time.perf_counter() - t0) * 1e3
    emit(index=f"ivfpq {n}x{D} nlist={nlist} M={M}", case=f"get_list of every list + host decode, {len(keys)} numpy keys", ms=round(ms_old, 1),
         reconstruct_batch_first_ms=round(ms_first, 2), reconstruct_batch_ms=round(ms_next, 2), equal=bool(np.array_equal(old.view(np.uint32), new.view(np.uint32))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-pq", type=int, default=100_000_000)
    ap.add_argument("--n-flat", type=int, default=10_000_000)
    ap.add_argument("--n-old", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch, rsx
    if args.n_old > 0:
        old_route(rsx, torch, args)
    if args.n_flat > 0:
        t0 = time.time()
        fx = rsx.IndexFlatIP(D, device=0)
        fill(rsx, torch, fx, args.n_flat)
        print(f"[bench_reconstruct] Flat build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        measure(rsx, torch, fx, f"flat {args.n_flat}x{D} IP", args.n_flat, args, False)
        del fx
        torch.cuda.empty_cache()
    if args.n_pq > 0:
        t0 = time.time()
        free, _ = torch.cuda.mem_get_info()
        fit = int((free - (40 << 30)) // (2 * args.m + 2 * 8))      # codes with their growth margin, ids; 40 GB left for maps, outputs, workspaces
        if fit < args.n_pq:
            args.n_pq = max(1_000_000, fit // 1_000_000 * 1_000_000)
            print(f"[bench_reconstruct] {free >> 30} GiB free: the IVF-PQ index holds {args.n_pq} vectors", file=sys.stderr, flush=True)
        ix = train_ivfpq(rsx, torch, args.n_pq, args.nlist, args.m)
        fill(rsx, torch, ix, args.n_pq)
        ix.nprobe = args.nprobe
        print(f"[bench_reconstruct] IVF-PQ build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        measure(rsx, torch, ix, f"ivfpq {args.n_pq}x{D} nlist={args.nlist} M={args.m} nprobe={args.nprobe}", args.n_pq, args, True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# reconstruct: measured on one MI355X (tools/bench_reconstruct.py)\n\n")
            f.write(f"Batch {args.batch}, CUDA tensors in and out, mean of {args.steps} calls after one warm-up; `out_TB_per_s` is output bytes per second, "
                    f"`of_hbm` its share of the {HBM_TBS} TB/s a streaming kernel reaches.\n\n")
            f.write("| index | case | ms | other figures |\n|---|---|---|---|\n")
            for r in ROWS:
                rest = "; ".join(f"{c} = {v}" for c, v in r.items() if c not in ("index", "case", "ms") and v is not None)
                f.write(f"| {r['index']} | {r['case']} | {'' if r.get('ms') is None else r['ms']} | {rest} |\n")

if __name__ == "__main__":
    main()
