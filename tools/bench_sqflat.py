#!/usr/bin/env python3
"""IndexScalarQuantizer measurement (profiles/indexsq_speed.md): the flat 8-bit scalar quantiser's int8 GEMM route against
  (a) an IndexIVFScalarQuantizer of ONE list with a zero centroid and by_residual off — the only way to get this search before the kind
      existed, and the route the new kind keeps for small batches, and
  (b) an IndexFlat (fp16 rows, k_flat_gemm2) over the same vectors,
in one process on one GPU — the bench generator's data (768 dimensions, NC 4096, seeds as bench.py), one JSON line per measurement.

  per index, metric and k   ms per batch of distinct queries (synchronised wall time: median, min, max over --steps batches after a
                            warm-up; --repeat runs of it: the spread of two runs is what a difference has to exceed), then a profiled
                            pass for the stage breakdown, the re-run queries and (scalar quantiser) the keys per query through the filter
  recall                    --recall Q: recall@10 of the first Q queries against the IndexFlat's result

  python tools/bench_sqflat.py [--n 10000000] [--ks 10,100,1000] [--metrics ip,l2] [--batch 1024] [--recall 256] [--skip a,b]
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


def measure(torch, ix, name, Q, args, k, extra, steps=None):
    steps = steps or args.steps
    timed(torch, ix, Q, args.batch, k, 0, args.warmup)
    runs = []
    for _ in range(args.repeat):
        ms = timed(torch, ix, Q, args.batch, k, args.warmup, steps)
        runs.append({"ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)})
    ix.set_param("profile", 2)
    ix.search(Q[:args.batch], k)
    st = {t: round(ix.get_timing(t), 4) for t in STAGES if ix.get_timing(t) > 0}
    rec = {"index": name, **extra, "k": k, "batch": args.batch, "steps": steps, "runs": runs, "stage_ms": st,
           "fallback_queries": ix.get_timing("fallback_queries"), "gemm_launches": ix.get_timing("sqflat_gemm_launches"),
           "stages": ix.get_timing("sqflat_stages"), "cand_keys_per_query": round(ix.get_timing("cand_keys") / args.batch, 1),
           "hbm_bytes": ix._get("hbm_bytes"), "workspace_bytes": ix._get("workspace_bytes")}
    ix.set_param("profile", 0)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--ks", default="10,100,1000")
    ap.add_argument("--metrics", default="ip,l2")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--steps-a", type=int, default=3, help="batches per run of baseline (a): its score rows make a batch many times slower")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--train", type=int, default=262144)
    ap.add_argument("--recall", type=int, default=0)
    ap.add_argument("--skip", default="", help="comma list of: a (the one-list IVF-SQ baseline), b (IndexFlat)")
    args = ap.parse_args()
    import torch, rsx
    skip = set(v for v in args.skip.split(",") if v)
    ks = [int(v) for v in args.ks.split(",") if v]
    n = args.n
    Q = torch.empty(((args.warmup + args.steps) * args.batch, D), dtype=torch.float16, device="cuda:0")
    rsx.synth_queries(D, NC, SC, SX, 0.5, n, SQ, 0.1, 0, Q.shape[0], out=Q)
    xt = torch.empty((min(args.train, n), D), dtype=torch.float16, device="cuda:0")
    rsx.synth_vectors(D, NC, SC, SX, 0.5, 0, xt.shape[0], out=xt)
    for mname in [v for v in args.metrics.split(",") if v]:
        metric = rsx.METRIC_L2 if mname == "l2" else rsx.METRIC_INNER_PRODUCT
        extra = {"n": n, "metric": mname}
        top = {}
        t0 = time.time()
        sq = rsx.IndexScalarQuantizer(D, rsx.ScalarQuantizer.QT_8bit, metric, device=0)
        sq.train(xt)
        trained = sq.sq.trained
        fill(rsx, torch, sq, n)
        print(f"[bench_sqflat] IndexScalarQuantizer {n} x {D} {mname} build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        for k in ks:
            measure(torch, sq, "IndexScalarQuantizer", Q, args, k, extra)
        if args.recall > 0:
            top["IndexScalarQuantizer"] = sq.search(Q[:args.recall], 10)[1].cpu().numpy()
        del sq
        torch.cuda.empty_cache()
        if "a" not in skip:
            t0 = time.time()
            one = rsx.IndexIVFScalarQuantizer(None, D, 1, rsx.ScalarQuantizer.QT_8bit, metric, False, device=0)
            one.set_centroids(np.zeros((1, D), np.float32))
            one.set_sq_trained(trained)
            fill(rsx, torch, one, n)
            print(f"[bench_sqflat] one-list IndexIVFScalarQuantizer build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
            for k in ks:
                measure(torch, one, "IndexIVFScalarQuantizer, one list", Q, args, k, extra, min(args.steps, args.steps_a))
            if args.recall > 0:
                top["IndexIVFScalarQuantizer, one list"] = one.search(Q[:args.recall], 10)[1].cpu().numpy()
            del one
            torch.cuda.empty_cache()
        if "b" not in skip or args.recall > 0:
            t0 = time.time()
            fl = rsx.IndexFlat(D, metric, device=0)
            fill(rsx, torch, fl, n)
            print(f"[bench_sqflat] IndexFlat build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
            if "b" not in skip:
                for k in ks:
                    measure(torch, fl, "IndexFlat", Q, args, k, extra)
            if args.recall > 0:
                gt = fl.search(Q[:args.recall], 10)[1].cpu().numpy()
                for name, I in top.items():
                    r = float(np.mean([len(set(I[i]) & set(gt[i])) / 10.0 for i in range(len(gt))]))
                    print(json.dumps({"recall_at_10": round(r, 4), "index": name, **extra, "queries": args.recall}), flush=True)
            del fl
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
