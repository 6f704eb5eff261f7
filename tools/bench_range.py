#!/usr/bin/env python3
"""Range-search measurement: ms per 1024-query batch of index.range_search on a 10M x 768 Flat index and on a 100M x 768
IVF-Flat index (nlist 4096, nprobe 32; fewer vectors when the free device memory does not hold them: the size is printed), for radii that give about 10 and about 1000 results per query, beside index.search at k = 10 and
k = 1000 on the same index in the same process as the yardstick.  The radii are found by bisection on the first batch's mean result
count.  Per case: results and candidates per query, overflowed queries, and the share of the back end
(re-score, ordering, emission) in the call's stream time.  One JSON line per (index, case) on stdout.

  python tools/bench_range.py [--n-flat 10000000] [--n-ivf 100000000] [--steps 5] [--warmup 1]
"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retrieval-scaling_amd")); sys.path.insert(0, REPO)
import numpy as np

D, NC, SC, SX, SQ = 768, 4096, 1234, 10000, 999


def fill(rsx, torch, ix, n, reserve=False):
    buf = torch.empty((1_000_000, D), dtype=torch.float16, device=torch.device("cuda", 0))
    if reserve:          # the lists' final sizes first: growing a 150 GB layout in place needs a second copy of it
        counts = np.zeros(ix.nlist, dtype=np.int64)
        for c0 in range(0, n, 1_000_000):
            nb = min(1_000_000, n - c0)
            rsx.synth_vectors(D, NC, SC, SX, 0.5, c0, nb, out=buf[:nb])
            counts += np.bincount(ix.assign(buf[:nb]), minlength=ix.nlist)
        ix.reserve_lists(counts)
    for c0 in range(0, n, 1_000_000):
        nb = min(1_000_000, n - c0)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, c0, nb, out=buf[:nb])
        ix.add(buf[:nb])
    del buf


def timed(torch, fn, Q, batch, steps, warmup):
    for i in range(warmup):
        fn(Q[i * batch:(i + 1) * batch])
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for i in range(warmup, warmup + steps):
        fn(Q[i * batch:(i + 1) * batch])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def radius_for(ix, Q0, target):
    """the radius at which the first batch has about `target` results per query on average: bisection between the batch's best score and
    the median score at rank 4 x target (inner product: more results as the radius falls)"""
    Dk, _ = ix.search(Q0, min(4096, 4 * target))
    hi, lo = float(Dk[:, 0].max().item()), float(Dk[:, -1].float().median().item())
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        mean = ix.range_search(Q0, mid)[0][-1].item() / len(Q0)
        if abs(mean - target) <= 0.05 * target:
            return mid
        if mean > target:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def run(torch, ix, name, Q, batch, steps, warmup, targets):
    keys = ("range_candidates", "range_results", "range_overflow_queries", "range_ms", "range_backend_ms")
    for k in targets:
        radius = radius_for(ix, Q[:batch], k)
        ms = timed(torch, lambda q: ix.search(q, k), Q, batch, steps, warmup)
        print(json.dumps({"index": name, "case": f"search k={k}", "batch": batch, "steps": steps, "ms_per_batch": round(ms, 3)}), flush=True)
        ms = timed(torch, lambda q: ix.range_search(q, radius), Q, batch, steps, warmup)
        ix.set_param("profile", 1)             # a separate, event-timed pass for the stage split
        t0 = {key: ix.get_timing(key) for key in keys}
        for i in range(warmup, warmup + steps):
            ix.range_search(Q[i * batch:(i + 1) * batch], radius)
        dt = {key: ix.get_timing(key) - t0[key] for key in keys}
        ix.set_param("profile", 0)
        nq = batch * steps
        print(json.dumps({"index": name, "case": f"range_search ~{k} results", "radius": radius, "batch": batch, "steps": steps,
                          "ms_per_batch": round(ms, 3), "results_per_query": round(dt["range_results"] / nq, 1),
                          "candidates_per_query": round(dt["range_candidates"] / nq, 1), "overflow_queries": dt["range_overflow_queries"],
                          "stream_ms_per_batch": round(dt["range_ms"] / steps, 3),
                          "backend_share": round(dt["range_backend_ms"] / max(dt["range_ms"], 1e-9), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-flat", type=int, default=10_000_000)
    ap.add_argument("--n-ivf", type=int, default=100_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--targets", type=int, nargs="+", default=[10, 1000], help="results per query to aim the radii at (= the k of the yardstick searches)")
    args = ap.parse_args()
    import torch, rsx
    nsteps = args.warmup + args.steps

    def queries(n):
        Q = torch.empty((nsteps * args.batch, D), dtype=torch.float16, device="cuda:0")
        rsx.synth_queries(D, NC, SC, SX, 0.5, n, SQ, 0.1, 0, nsteps * args.batch, out=Q)
        return Q
    if args.n_flat > 0:
        t0 = time.time()
        fx = rsx.IndexFlatIP(D, device=0)
        fill(rsx, torch, fx, args.n_flat)
        print(f"[bench_range] Flat build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        run(torch, fx, f"flat {args.n_flat}x{D} IP", queries(args.n_flat), args.batch, args.steps, args.warmup, args.targets)
        del fx
        torch.cuda.empty_cache()
    if args.n_ivf > 0:
        t0 = time.time()
        free, _ = torch.cuda.mem_get_info()
        fit = int((free - (24 << 30)) // (2 * D + 12))          # fp16 rows, ids, norms; 24 GB left for the workspaces
        if fit < args.n_ivf:
            args.n_ivf = max(1_000_000, fit // 1_000_000 * 1_000_000)
            print(f"[bench_range] {free >> 30} GiB free: the IVF-Flat index holds {args.n_ivf} vectors", file=sys.stderr, flush=True)
        ix = rsx.IndexIVFFlat(rsx.IndexFlatIP(D), D, args.nlist, rsx.METRIC_INNER_PRODUCT, device=0)
        nt = min(args.n_ivf, 256 * args.nlist)
        xt = torch.empty((nt, D), dtype=torch.float16, device="cuda:0")
        stride = max(1, args.n_ivf // nt)
        for b in range(0, nt, 4096):
            nb = min(4096, nt - b)
            rsx.synth_vectors(D, NC, SC, SX, 0.5, (b * stride) % max(1, args.n_ivf - nb), nb, out=xt[b:b + nb])
        ix.train(xt)
        del xt
        fill(rsx, torch, ix, args.n_ivf, reserve=True)
        ix.nprobe = args.nprobe
        print(f"[bench_range] IVF-Flat build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        run(torch, ix, f"ivfflat {args.n_ivf}x{D} IP nlist={args.nlist} nprobe={args.nprobe}", queries(args.n_ivf), args.batch, args.steps,
            args.warmup, args.targets)


if __name__ == "__main__":
    main()
