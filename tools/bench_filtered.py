#!/usr/bin/env python3
"""Filtered-search measurement: queries/s per 1024-query batch of rsx_search_sel on the headline 100M x 768 IVF-PQ
index and on a 10M x 768 Flat index, for no selector, an all-pass selector, 50 / 10 / 1 % random selections (seeded bitmaps) and
a 10 % id range; the one-off slot-mask build time of every selector and the exact re-runs (fallback_queries / fast_queries) of
every case.  One JSON line per (index, case) on stdout.

  python tools/bench_filtered.py [--n-ivfpq 100000000] [--n-flat 10000000] [--steps 5] [--warmup 1]
"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retrieval-scaling_amd")); sys.path.insert(0, REPO)
import numpy as np

D, NC, SC, SX, SQ = 768, 4096, 1234, 10000, 999


def build_ivfpq(rsx, torch, n, nlist, m):
    dev = torch.device("cuda", 0)
    ix = rsx.IndexIVFPQ(rsx.IndexFlatIP(D), D, nlist, m, 8, rsx.METRIC_INNER_PRODUCT, device=0)
    nt = min(n, 256 * nlist)
    xt = torch.empty((nt, D), dtype=torch.float16, device=dev)
    stride = max(1, n // nt)
    for b in range(0, nt, 4096):
        nb = min(4096, nt - b)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, (b * stride) % max(1, n - nb), nb, out=xt[b:b + nb])
    ix.train(xt)
    del xt
    fill(rsx, torch, ix, n)
    return ix


def fill(rsx, torch, ix, n):
    buf = torch.empty((1_000_000, D), dtype=torch.float16, device=torch.device("cuda", 0))
    for c0 in range(0, n, 1_000_000):
        nb = min(1_000_000, n - c0)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, c0, nb, out=buf[:nb])
        ix.add(buf[:nb])
    del buf


def cases(rsx, n):
    rng = np.random.default_rng(2024)
    u = rng.random(n, dtype=np.float32)
    out = [("none", None), ("all_pass", rsx.IDSelectorRange(0, n))]
    for p in (0.5, 0.1, 0.01):
        out.append((f"random_{int(p * 100)}pct", rsx.IDSelectorBitmap(np.packbits(u < p, bitorder="little"))))
    out.append(("range_10pct", rsx.IDSelectorRange(int(0.45 * n), int(0.55 * n))))
    return out


def run(rsx, torch, ix, name, n, Q, batch, k, steps, warmup, ivf):
    for case, sel in cases(rsx, n):
        params = None
        if sel is not None:
            params = rsx.SearchParametersIVF(sel=sel, nprobe=ix.nprobe) if ivf else rsx.SearchParameters(sel=sel)
        t = {key: ix.get_timing(key) for key in ("sel_mask_builds", "sel_mask_ms", "fallback_queries", "fast_queries", "filtered_queries")}
        srch = (lambda q: ix.search(q, k)) if params is None else (lambda q: ix.search(q, k, params=params))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        srch(Q[:batch])                                  # the first batch builds the selector's mask
        torch.cuda.synchronize(); first_ms = (time.perf_counter() - t0) * 1e3
        for i in range(1, warmup):
            srch(Q[i * batch:(i + 1) * batch])
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(warmup, warmup + steps):
            srch(Q[i * batch:(i + 1) * batch])
        torch.cuda.synchronize(); el = time.perf_counter() - t0
        dt = {key: ix.get_timing(key) - v for key, v in t.items()}
        rec = {"index": name, "case": case, "k": k, "batch": batch, "steps": steps,
               "ms_per_batch": round(el * 1e3 / steps, 3), "queries_per_s": round(batch * steps / el, 1),
               "first_batch_ms": round(first_ms, 3), "mask_builds": dt["sel_mask_builds"], "mask_build_ms": round(dt["sel_mask_ms"], 3),
               "fast_queries": dt["fast_queries"], "fallback_queries": dt["fallback_queries"], "filtered_queries": dt["filtered_queries"]}
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ivfpq", type=int, default=100_000_000)
    ap.add_argument("--n-flat", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--pq-layout", type=int, default=None, help="rsx_set_param pq_layout of the IVF-PQ index (default: the library's)")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch, rsx
    nsteps = args.warmup + args.steps
    if args.n_ivfpq > 0:
        t0 = time.time()
        ix = build_ivfpq(rsx, torch, args.n_ivfpq, args.nlist, args.m) if args.pq_layout is None else None
        if ix is None:
            ix = rsx.IndexIVFPQ(rsx.IndexFlatIP(D), D, args.nlist, args.m, 8, rsx.METRIC_INNER_PRODUCT, device=0)
            ix.set_param("pq_layout", float(args.pq_layout))
            ref = build_ivfpq(rsx, torch, min(args.n_ivfpq, 256 * args.nlist), args.nlist, args.m)
            ix.set_centroids(ref.get_centroids()); ix.set_codebooks(ref.get_codebooks()); del ref
            fill(rsx, torch, ix, args.n_ivfpq)
        ix.nprobe = args.nprobe
        print(f"[bench_filtered] IVF-PQ build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        Q = torch.empty((nsteps * args.batch, D), dtype=torch.float16, device="cuda:0")
        rsx.synth_queries(D, NC, SC, SX, 0.5, args.n_ivfpq, SQ, 0.1, 0, nsteps * args.batch, out=Q)
        name = f"ivfpq {args.n_ivfpq}x{D} M={args.m} nlist={args.nlist} nprobe={args.nprobe} layout={ix._get('pq_layout')}"
        run(rsx, torch, ix, name, args.n_ivfpq, Q, args.batch, args.k, args.steps, args.warmup, True)
        del ix, Q
        torch.cuda.empty_cache()
    if args.n_flat > 0:
        t0 = time.time()
        fx = rsx.IndexFlatIP(D, device=0)
        fill(rsx, torch, fx, args.n_flat)
        print(f"[bench_filtered] Flat build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        Q = torch.empty((nsteps * args.batch, D), dtype=torch.float16, device="cuda:0")
        rsx.synth_queries(D, NC, SC, SX, 0.5, args.n_flat, SQ, 0.1, 0, nsteps * args.batch, out=Q)
        run(rsx, torch, fx, f"flat {args.n_flat}x{D} IP", args.n_flat, Q, args.batch, args.k, args.steps, args.warmup, False)


if __name__ == "__main__":
    main()
