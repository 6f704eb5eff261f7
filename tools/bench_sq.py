#!/usr/bin/env python3
"""IndexIVFScalarQuantizer measurement (profiles/ivfsq_speed.md): the 8-bit scalar-quantised IVF index against IndexIVFFlat
over the same vectors and centroids, in one process on one GPU — the bench generator's data (768 dimensions, NC 4096, seeds as
bench.py), inner product or L2, one JSON line per measurement on stdout.

  per index and k   ms per batch of distinct queries (synchronised wall time: median, min, max over --steps batches after a warm-up),
                    then profiled passes for the stage breakdown, the fallbacks, the vectors the batch scans (unique per list) and from
                    them the scan's share of the HBM peak on unique bytes (row bytes x unique vectors / scan time / --hbm-peak)
  recall            --recall Q: recall@10 of the first Q queries against exact ground truth (an IndexFlat over the same vectors)
  sweep             --sweep-nprobe 16,32,64,128 [--sweep-qtiles 0,4]: instead of the headline measurement, the first k at every nprobe (the
                    probing queries per list grow with it while the unique bytes stay: what a (query, row) pair costs on the CU side) and,
                    for the scalar-quantiser index, with the 16-query (ivf_qtiles 0) and the 64-query (4) group form forced
  the two indexes are built one after the other (100M x 768 fp16 rows alone are 153.6 GB)

  python tools/bench_sq.py [--n 20000000] [--nlist 2048] [--nprobe 128] [--ks 10,1000] [--metric ip|l2] [--by-residual 1] [--recall 256]
"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retrieval-scaling_amd")); sys.path.insert(0, REPO)
import numpy as np

D, NC, SC, SX, SQ = 768, 4096, 1234, 10000, 999
CH = 1_000_000
STAGES = ("convert", "coarse", "select_probe", "sq_factors", "group", "scan0", "select0", "scan", "select", "finalize", "total")


def fill(rsx, torch, ix, n):
    buf = torch.empty((CH, D), dtype=torch.float16, device="cuda:0")
    for c0 in range(0, n, CH):
        nb = min(CH, n - c0)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, c0, nb, out=buf[:nb])
        ix.add(buf[:nb])
    del buf


def timed(torch, ix, Q, batch, k, first, steps):
    out = []
    for i in range(first, first + steps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        ix.search(Q[i * batch:(i + 1) * batch], k)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def measure(torch, ix, name, Q, args, k, row_bytes, extra):
    timed(torch, ix, Q, args.batch, k, 0, args.warmup)
    ms = timed(torch, ix, Q, args.batch, k, args.warmup, args.steps)
    ix.set_param("profile", 1)
    ix.search(Q[:args.batch], k)
    st = {t: round(ix.get_timing(t), 4) for t in STAGES if ix.get_timing(t) > 0}
    fb = ix.get_timing("fallback_queries")
    ix.set_param("profile", 2)
    ix.search(Q[:args.batch], k)
    uniq = ix.get_timing("scanned_unique_vectors")
    ix.set_param("profile", 0)
    scan_ms = st.get("scan", 0.0) + st.get("scan0", 0.0)
    rec = {"index": name, **extra, "k": k, "batch": args.batch, "steps": args.steps, "ms_median": round(float(np.median(ms)), 3),
           "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "stage_ms": st, "fallback_queries": fb,
           "scanned_unique_vectors": uniq, "hbm_share_unique_bytes": round(uniq * row_bytes / (scan_ms * 1e-3) / args.hbm_peak, 3) if scan_ms > 0 else None,
           "hbm_bytes": ix._get("hbm_bytes")}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000_000)
    ap.add_argument("--nlist", type=int, default=2048)
    ap.add_argument("--nprobe", type=int, default=128)
    ap.add_argument("--ks", default="10,1000")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--metric", choices=("ip", "l2"), default="ip")
    ap.add_argument("--by-residual", type=int, default=1)
    ap.add_argument("--train", type=int, default=262144)
    ap.add_argument("--recall", type=int, default=0, help="queries whose recall@10 against exact ground truth is reported (builds an IndexFlat)")
    ap.add_argument("--hbm-peak", type=float, default=8.0e12, help="bytes per second the share is taken of")
    ap.add_argument("--skip-flat", action="store_true", help="only the scalar-quantiser index")
    ap.add_argument("--sweep-nprobe", default="", help="nprobe values of the sweep (replaces the headline measurement)")
    ap.add_argument("--sweep-qtiles", default="0,4", help="ivf_qtiles values forced on the scalar-quantiser index in the sweep")
    args = ap.parse_args()
    import torch, rsx
    metric = rsx.METRIC_L2 if args.metric == "l2" else rsx.METRIC_INNER_PRODUCT
    ks = [int(v) for v in args.ks.split(",") if v]
    n = args.n
    extra = {"n": n, "nlist": args.nlist, "nprobe": args.nprobe, "metric": args.metric}
    Q = torch.empty(((args.warmup + args.steps) * args.batch, D), dtype=torch.float16, device="cuda:0")
    rsx.synth_queries(D, NC, SC, SX, 0.5, n, SQ, 0.1, 0, Q.shape[0], out=Q)
    xt = torch.empty((min(args.train, n), D), dtype=torch.float16, device="cuda:0")
    rsx.synth_vectors(D, NC, SC, SX, 0.5, 0, xt.shape[0], out=xt)

    t0 = time.time()
    sq = rsx.IndexIVFScalarQuantizer(None, D, args.nlist, rsx.ScalarQuantizer.QT_8bit, metric, bool(args.by_residual), device=0)
    sq.train(xt)
    cen = sq.get_centroids()
    fill(rsx, torch, sq, n)
    sizes = sq.list_sizes()
    sq.nprobe = args.nprobe
    print(f"[bench_sq] IndexIVFScalarQuantizer {n} x {D} nlist {args.nlist} build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    top = {}
    sweep = [int(v) for v in args.sweep_nprobe.split(",") if v]

    def run_sweep(ix, name, row_bytes, qtiles):
        for npb in sweep:
            ix.nprobe = npb
            for qt in qtiles:
                ix.set_param("ivf_qtiles", float(qt))
                measure(torch, ix, name, Q, args, ks[0], row_bytes, {**extra, "nprobe": npb, "ivf_qtiles": qt,
                                                                     "probing_queries_per_list": round(args.batch * min(npb, args.nlist) / args.nlist, 1)})
        ix.set_param("ivf_qtiles", 1.0)
        ix.nprobe = args.nprobe
    if sweep:
        run_sweep(sq, "IndexIVFScalarQuantizer", D, [int(v) for v in args.sweep_qtiles.split(",") if v])
    for k in ([] if sweep else ks):
        measure(torch, sq, "IndexIVFScalarQuantizer", Q, args, k, D, {**extra, "by_residual": args.by_residual})
    if args.recall > 0:
        top["sq"] = sq.search(Q[:args.recall], 10)[1].cpu().numpy()
    del sq
    torch.cuda.empty_cache()

    if not args.skip_flat:
        t0 = time.time()
        fl = rsx.IndexIVFFlat(None, D, args.nlist, metric, device=0)
        fl.set_centroids(cen)
        fl.reserve_lists(sizes)      # same centroids, same membership: one allocation (a growth re-layout of 153.6 GB of rows would not fit beside itself)
        fill(rsx, torch, fl, n)
        fl.nprobe = args.nprobe
        print(f"[bench_sq] IndexIVFFlat {n} x {D} nlist {args.nlist} build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        if sweep:
            run_sweep(fl, "IndexIVFFlat", 2 * D, [1])
        for k in ([] if sweep else ks):
            measure(torch, fl, "IndexIVFFlat", Q, args, k, 2 * D, extra)
        if args.recall > 0:
            top["ivfflat"] = fl.search(Q[:args.recall], 10)[1].cpu().numpy()
        del fl
        torch.cuda.empty_cache()

    if args.recall > 0:
        ex = rsx.IndexFlat(D, metric, device=0)
        fill(rsx, torch, ex, n)
        gt = ex.search(Q[:args.recall], 10)[1].cpu().numpy()
        del ex
        for name, I in top.items():
            r = float(np.mean([len(set(I[i]) & set(gt[i])) / 10.0 for i in range(len(gt))]))
            print(json.dumps({"recall_at_10": round(r, 4), "index": name, **extra, "queries": args.recall}), flush=True)


if __name__ == "__main__":
    main()
