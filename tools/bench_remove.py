#!/usr/bin/env python3
"""remove_ids measurement: host wall time of Index.remove_ids (mask build, plan, moves, clearing, directory upload)
for 1 / 10 / 50 % random ids and one 10 % id range, on the headline 100M x 768 IVF-PQ index (M = 96, sliced and rotated layouts),
a 100M x 768 IVF-Flat index and a 10M x 768 Flat IP index, synthetic data as in bench.py.  Every case starts from a full index
(reset + refill: trained parameters and list reservations are kept).  After the 1 % removal it also times the search per
1024-query batch, next to the filtered search with IDSelectorNot of the same ids on the index before the removal.  One JSON line
per (index, case) on stdout.

  python tools/bench_remove.py [--n-ivfpq 100000000] [--n-ivfflat 100000000] [--n-flat 10000000] [--steps 5] [--warmup 1]
"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retrieval-scaling_amd")); sys.path.insert(0, REPO)
import numpy as np

D, NC, SC, SX, SQ = 768, 4096, 1234, 10000, 999
CH = 1_000_000


def _buf(torch):
    return torch.empty((CH, D), dtype=torch.float16, device=torch.device("cuda", 0))


def fill(rsx, torch, ix, n):
    buf = _buf(torch)
    for c0 in range(0, n, CH):
        nb = min(CH, n - c0)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, c0, nb, out=buf[:nb])
        ix.add(buf[:nb])
    del buf


def train(rsx, torch, ix, n, nlist):
    nt = min(n, 256 * nlist)
    xt = torch.empty((nt, D), dtype=torch.float16, device=torch.device("cuda", 0))
    stride = max(1, n // nt)
    for b in range(0, nt, 4096):
        nb = min(4096, nt - b)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, (b * stride) % max(1, n - nb), nb, out=xt[b:b + nb])
    ix.train(xt)
    del xt


def reserve_exact(rsx, torch, ix, n, nlist):
    """list sizes first (rsx_assign), then one exact reservation: a 100M IVF-Flat index cannot hold two copies of itself"""
    counts = np.zeros(nlist, np.int64)
    buf = _buf(torch)
    for c0 in range(0, n, CH):
        nb = min(CH, n - c0)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, c0, nb, out=buf[:nb])
        counts += np.bincount(np.asarray(ix.assign(buf[:nb])).reshape(-1), minlength=nlist)
    del buf
    ix.reserve_lists(counts)


def cases(rsx, n):
    rng = np.random.default_rng(2024)
    out = []
    for p in (0.01, 0.1, 0.5):
        out.append((f"random_{int(p * 100)}pct", np.sort(rng.choice(n, int(p * n), replace=False)).astype(np.int64)))
    out.append(("range_10pct", (int(0.45 * n), int(0.55 * n))))
    return out


def time_search(torch, srch, Q, batch, steps, warmup):
    for i in range(warmup):
        srch(Q[i * batch:(i + 1) * batch])
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for i in range(warmup, warmup + steps):
        srch(Q[i * batch:(i + 1) * batch])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def run(rsx, torch, ix, name, n, Q, args, ivf):
    k, batch = args.k, args.batch
    for i, (case, ids) in enumerate(cases(rsx, n)):
        if i:
            ix.reset()
            fill(rsx, torch, ix, n)
        sel = rsx.IDSelectorRange(*ids) if case.startswith("range") else rsx.IDSelectorBatch(ids)
        rec = {"index": name, "case": case, "ntotal": ix.ntotal}
        if case == "random_1pct":
            notp = rsx.IDSelectorNot(sel)
            params = rsx.SearchParametersIVF(sel=notp, nprobe=ix.nprobe) if ivf else rsx.SearchParameters(sel=notp)
            rec["search_ms_unremoved"] = round(time_search(torch, lambda q: ix.search(q, k), Q, batch, args.steps, args.warmup), 3)
            rec["filtered_not_ms"] = round(time_search(torch, lambda q: ix.search(q, k, params=params), Q, batch, args.steps, args.warmup), 3)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        nrm = ix.remove_ids(sel)
        rec["remove_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        rec["removed"] = nrm
        if case == "random_1pct":
            rec["search_ms_after_remove"] = round(time_search(torch, lambda q: ix.search(q, k), Q, batch, args.steps, args.warmup), 3)
        rec["k"], rec["batch"], rec["steps"] = k, batch, args.steps
        print(json.dumps(rec), flush=True)


def queries(rsx, torch, n, args):
    Q = torch.empty(((args.warmup + args.steps) * args.batch, D), dtype=torch.float16, device="cuda:0")
    rsx.synth_queries(D, NC, SC, SX, 0.5, n, SQ, 0.1, 0, Q.shape[0], out=Q)
    return Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ivfpq", type=int, default=100_000_000)
    ap.add_argument("--n-ivfflat", type=int, default=100_000_000)
    ap.add_argument("--n-flat", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--layouts", default="2,1", help="IVF-PQ code layouts to measure (rsx_set_param pq_layout)")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch, rsx
    if args.n_ivfpq > 0:
        cen = cb = None
        for layout in [int(v) for v in args.layouts.split(",") if v]:
            t0 = time.time()
            ix = rsx.IndexIVFPQ(rsx.IndexFlatIP(D), D, args.nlist, args.m, 8, rsx.METRIC_INNER_PRODUCT, device=0)
            ix.set_param("pq_layout", float(layout))
            if cen is None:
                train(rsx, torch, ix, args.n_ivfpq, args.nlist)
                cen, cb = ix.get_centroids(), ix.get_codebooks()
            else:
                ix.set_centroids(cen); ix.set_codebooks(cb)
            fill(rsx, torch, ix, args.n_ivfpq)
            ix.nprobe = args.nprobe
            print(f"[bench_remove] IVF-PQ layout {layout} build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
            Q = queries(rsx, torch, args.n_ivfpq, args)
            run(rsx, torch, ix, f"ivfpq {args.n_ivfpq}x{D} M={args.m} nlist={args.nlist} nprobe={args.nprobe} layout={layout}", args.n_ivfpq,
                Q, args, True)
            del ix, Q
            torch.cuda.empty_cache()
    if args.n_ivfflat > 0:
        t0 = time.time()
        ix = rsx.IndexIVFFlat(rsx.IndexFlatIP(D), D, args.nlist, rsx.METRIC_INNER_PRODUCT, device=0)
        train(rsx, torch, ix, args.n_ivfflat, args.nlist)
        reserve_exact(rsx, torch, ix, args.n_ivfflat, args.nlist)
        fill(rsx, torch, ix, args.n_ivfflat)
        ix.nprobe = args.nprobe
        print(f"[bench_remove] IVF-Flat build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        Q = queries(rsx, torch, args.n_ivfflat, args)
        run(rsx, torch, ix, f"ivfflat {args.n_ivfflat}x{D} nlist={args.nlist} nprobe={args.nprobe}", args.n_ivfflat, Q, args, True)
        del ix, Q
        torch.cuda.empty_cache()
    if args.n_flat > 0:
        t0 = time.time()
        fx = rsx.IndexFlatIP(D, device=0)
        fill(rsx, torch, fx, args.n_flat)
        print(f"[bench_remove] Flat build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        Q = queries(rsx, torch, args.n_flat, args)
        run(rsx, torch, fx, f"flat {args.n_flat}x{D} IP", args.n_flat, Q, args, False)


if __name__ == "__main__":
    main()
