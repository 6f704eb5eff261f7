#!/usr/bin/env python3
"""IndexPQ measurement (profiles/indexpq_speed.md): the staged filtered scan of a flat product quantiser on the bench
generator's data (768 dimensions, NC 4096, seeds as bench.py), inner product or (--metric l2, profiles/indexpq_l2_speed.md) L2, one JSON
line per measurement on stdout.

  headline   per (n, M[, layout]) and k: ms per batch of distinct queries (synchronised wall time: median, min, max over --steps
             batches after a warm-up of the shape), then one profiled pass for the stage breakdown ("lut8", "scan0", "scan", "select",
             "finalize"), the stages, the survivors per query (rows of the candidate rows: mean, max), the fallbacks and the scan's
             (query, vector) pairs per second = batch x n / scan time
  emulation  --emulation: the one-list IndexIVFPQ (nlist 1, zero centroid, nprobe 1: code that needs no IndexPQ) holding the same
             codes and codebooks, alternated with IndexPQ in one process, --repeats repeats of --steps batches each; the pass
             condition of profiles/indexpq_speed.md is IndexPQ's slowest repeat against the emulation's fastest

  check      --check Q: the first Q queries' staged result against the exact scan (pq_fast = 0) of the same index, either metric
  exact      --pq-fast 0: time the exact scan itself (under L2 the route every L2 IndexPQ took before the staged scan served both metrics)

  python tools/bench_pq.py [--n 10000000] [--ms 64,96] [--ks 10,100,1000] [--layouts 96:2,96:1] [--emulation] [--check 32] [--steps 20] [--metric ip|l2]
"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retrieval-scaling_amd")); sys.path.insert(0, REPO)
import numpy as np

D, NC, SC, SX, SQ = 768, 4096, 1234, 10000, 999
CH = 1_000_000


def build(rsx, torch, n, M, layout, cb=None, metric=0):
    dev = torch.device("cuda", 0)
    ix = rsx.IndexPQ(D, M, 8, metric, device=0)
    if layout is not None:
        ix.set_param("pq_layout", float(layout))
    if cb is None:
        xt = torch.empty((65536, D), dtype=torch.float16, device=dev)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, 0, 65536, out=xt)
        ix.train(xt)
        del xt
    else:
        ix.set_codebooks(cb)
    buf = torch.empty((CH, D), dtype=torch.float16, device=dev)
    for c0 in range(0, n, CH):
        nb = min(CH, n - c0)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, c0, nb, out=buf[:nb])
        ix.add(buf[:nb])
    del buf
    return ix


def queries(rsx, torch, n, nbatches, batch):
    Q = torch.empty((nbatches * batch, D), dtype=torch.float16, device="cuda:0")
    rsx.synth_queries(D, NC, SC, SX, 0.5, n, SQ, 0.1, 0, Q.shape[0], out=Q)
    return Q


def timed(torch, ix, Q, batch, k, first, steps):
    """ms of each of `steps` batches (distinct queries), synchronised wall time"""
    out = []
    for i in range(first, first + steps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        ix.search(Q[i * batch:(i + 1) * batch], k)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def profile_pass(torch, ix, Q, batch, k, n):
    ix.set_param("profile", 1)
    ix.search(Q[:batch], k)
    st = {t: round(ix.get_timing(t), 4) for t in ("convert", "coarse", "select_probe", "lut8", "scan0", "scan", "select", "finalize", "total")}
    stages, fb = ix.get_timing("pq_flat_stages"), ix.get_timing("fallback_queries")
    ix.set_param("profile", 2)
    ix.search(Q[:batch], k)
    keys, kmax = ix.get_timing("cand_keys"), ix.get_timing("cand_keys_max")
    ix.set_param("profile", 0)
    return {"stage_ms": st, "stages": stages, "fallback_queries": fb, "cand_keys_mean": round(keys / batch, 1), "cand_keys_max": kmax,
            "scan_pairs_per_s": (batch * n / (st["scan"] * 1e-3)) if st["scan"] > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="10000000")
    ap.add_argument("--ms", default="64,96")
    ap.add_argument("--ks", default="10,100,1000")
    ap.add_argument("--layouts", default="", help="M:layout pairs to measure instead of the default layout of an M, e.g. 96:2,96:1")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--emulation", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--metric", choices=("ip", "l2"), default="ip")
    ap.add_argument("--pq-fast", type=int, default=1, help="0: time the exact scan (no --check then)")
    ap.add_argument("--check", type=int, default=0, help="queries of the first batch whose staged result is compared with the exact scan (pq_fast = 0)")
    args = ap.parse_args()
    import torch, rsx
    metric = rsx.METRIC_L2 if args.metric == "l2" else rsx.METRIC_INNER_PRODUCT
    tag = {} if (args.metric == "ip" and args.pq_fast == 1) else {"metric": args.metric, "pq_fast": args.pq_fast}      # (the default run's lines are unchanged)
    ks = [int(v) for v in args.ks.split(",") if v]
    shapes = [(int(m), None) for m in args.ms.split(",") if m]
    if args.layouts:
        shapes = [(int(p.split(":")[0]), int(p.split(":")[1])) for p in args.layouts.split(",") if p]
    for n in [int(v) for v in args.n.split(",") if v]:
        Q = queries(rsx, torch, n, args.warmup + args.steps, args.batch)
        for M, layout in shapes:
            t0 = time.time()
            ix = build(rsx, torch, n, M, layout, metric=metric)
            print(f"[bench_pq] IndexPQ {n} x {D} M={M} layout={ix._get('pq_layout')} build {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
            if args.check > 0 and args.pq_fast == 1:      # the exact scan addresses rows with 64-bit offsets and shares nothing with the staged route but the codes
                Df, If = ix.search(Q[:args.batch], ks[0])
                ix.set_param("pq_fast", 0)
                De, Ie = ix.search(Q[:args.check], ks[0])
                ix.set_param("pq_fast", 1)
                print(json.dumps({"check": "staged scan vs exact scan", **tag, "n": n, "M": M, "k": ks[0], "queries": args.check,
                                  "same_result": bool(torch.equal(Df[:args.check], De) and torch.equal(If[:args.check], Ie))}), flush=True)
            if args.pq_fast != 1:
                ix.set_param("pq_fast", float(args.pq_fast))
            for k in ks:
                timed(torch, ix, Q, args.batch, k, 0, args.warmup)
                ms = timed(torch, ix, Q, args.batch, k, args.warmup, args.steps)
                rec = {"index": "IndexPQ", **tag, "n": n, "M": M, "pq_layout": ix._get("pq_layout"), "k": k, "batch": args.batch, "steps": args.steps,
                       "ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}
                rec.update(profile_pass(torch, ix, Q, args.batch, k, n))
                print(json.dumps(rec), flush=True)
            if args.emulation and M == 64:
                k = ks[0]
                em = rsx.IndexIVFPQ(rsx.IndexFlatIP(D), D, 1, M, 8, metric, device=0)
                em.set_centroids(np.zeros((1, D), np.float32)); em.set_codebooks(ix.get_codebooks())
                codes, ids = ix.get_list(0)
                em.add_list(0, codes, ids); em.nprobe = 1
                del codes, ids
                De, Ie = em.search(Q[:args.batch], k); Dp, Ip = ix.search(Q[:args.batch], k)
                same = bool(torch.equal(De, Dp) and torch.equal(Ie, Ip))
                steps = max(1, min(args.steps, 4))
                timed(torch, em, Q, args.batch, k, 0, 1); timed(torch, ix, Q, args.batch, k, 0, 1)
                reps = {"emulation": [], "IndexPQ": []}
                for r in range(args.repeats):
                    for name, obj in (("emulation", em), ("IndexPQ", ix)):
                        reps[name].append(round(float(np.mean(timed(torch, obj, Q, args.batch, k, args.warmup, steps))), 3))
                print(json.dumps({"comparison": "one-list IndexIVFPQ vs IndexPQ", "n": n, "M": M, "k": k, "batch": args.batch, "batches_per_repeat": steps,
                                  "same_result": same, "emulation_ms": reps["emulation"], "indexpq_ms": reps["IndexPQ"],
                                  "pass": max(reps["IndexPQ"]) < min(reps["emulation"]),
                                  "ratio_fastest_emulation_over_slowest_indexpq": round(min(reps["emulation"]) / max(reps["IndexPQ"]), 2)}), flush=True)
                del em
            del ix
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
