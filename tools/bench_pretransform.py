#!/usr/bin/env python3
"""Transform-layer measurement, on one MI355X:
  * rsx_vt_apply alone, CUDA tensors in and out: 1024 x 768 -> 768 and 1024 x 768 -> 256 (a query batch; fp16 and fp32 input), and a
    1M x 768 -> 768 block (what `add` pays), as ms per call (host clock around calls that end in the library's stream synchronisation)
    and as FLOP/s of the 2 n d_in d_out operations the contraction needs;
  * `search` of a 1024-query batch through IndexPreTransform(OPQMatrix, IndexIVFPQ) against the SAME base index searched with queries
    rotated beforehand — the two alternate inside one loop, the difference is the feature's whole added cost;
  * `add` throughput through the transform and into an identical base without it;
  * recall@10 of the IVF-PQ index with and without OPQ against the exact Flat search of the raw rows, on the informative mixture
    (n / 8 centres, sigma 0.1) and on the standard one.
One JSON line per case on stdout; --out writes them as a markdown table.

  python tools/bench_pretransform.py [--n 10000000] [--nlist 4096] [--m 96] [--nprobe 32] [--opq-niter 4] [--steps 20] [--out FILE]
"""
import argparse, ctypes, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retrieval-scaling_amd")); sys.path.insert(0, REPO)
import numpy as np

D, NC, SC, SX, SQ = 768, 4096, 1234, 10000, 999
ROWS = []


def emit(**kw):
    ROWS.append(kw)
    print(json.dumps(kw), flush=True)


def ms_of(torch, fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def apply_cases(rsx, torch, args):
    for n, d_out, dtype, steps in ((1024, 768, torch.float16, 500), (1024, 768, torch.float32, 500), (1024, 256, torch.float16, 500),
                                   (1_000_000, 768, torch.float16, 10)):
        vt = rsx.RandomRotationMatrix(D, d_out)
        vt.init(1)
        x = torch.randn((n, D), device="cuda:0").to(dtype)
        ms = ms_of(torch, lambda: vt.apply(x), steps)
        emit(case=f"apply {n} x {D} -> {d_out}, {str(dtype).split('.')[-1]} in", ms=round(ms, 4), calls=steps,
             tflops=round(2.0 * n * D * d_out / (ms * 1e-3) / 1e12, 2))
        del x, vt


def synth_block(rsx, torch, nc, sig, c0, nb, buf):
    rsx.synth_vectors(D, nc, SC, SX, sig, c0, nb, out=buf[:nb])
    return buf[:nb]


def index_cases(rsx, torch, args, mixture):
    n, k, nq = args.n, 10, args.batch
    nc, sig, sigq = (max(1, n // 8), 0.1, 0.02) if mixture == "informative" else (NC, 0.5, 0.1)
    name = f"{mixture} mixture, {n} x {D}, IVF{args.nlist},PQ{args.m}, nprobe {args.nprobe}"
    nt = min(n, 256 * args.nlist)
    xt = torch.empty((nt, D), dtype=torch.float16, device="cuda:0")
    stride = max(1, n // nt)
    for b in range(0, nt, 4096):
        nb = min(4096, nt - b)
        rsx.synth_vectors(D, nc, SC, SX, sig, (b * stride) % max(1, n - nb), nb, out=xt[b:b + nb])
    plain = rsx.IndexIVFPQ(None, D, args.nlist, args.m, 8, rsx.METRIC_INNER_PRODUCT, device=0)
    plain.train(xt)
    opq = rsx.OPQMatrix(D, args.m)
    opq.niter = args.opq_niter
    pt = rsx.IndexPreTransform(opq, rsx.IndexIVFPQ(None, D, args.nlist, args.m, 8, rsx.METRIC_INNER_PRODUCT, device=0))
    t0 = time.perf_counter(); opq.train(xt); t_opq = time.perf_counter() - t0
    t0 = time.perf_counter(); pt.train(xt); t_tr = time.perf_counter() - t0
    emit(case=f"{name}: OPQMatrix.train, {min(nt, opq.max_train_points)} vectors, {opq.niter} iterations", ms=round(t_opq * 1e3, 1),
         pq_error_first=round(opq.pq_errors[0], 5), pq_error_last=round(opq.pq_errors[-1], 5), base_train_ms=round(t_tr * 1e3, 1))
    del xt
    flat = rsx.IndexFlatIP(D, device=0)      # exact ground truth; sized once (growing a row store of this size would need two copies of it)
    rsx._check(rsx.lib().rsx_reserve_lists(flat._h, np.array([n], dtype=np.int64).ctypes.data_as(ctypes.c_void_p)))
    buf = torch.empty((1_000_000, D), dtype=torch.float16, device="cuda:0")
    t_plain = t_pt = 0.0
    for c0 in range(0, n, buf.shape[0]):
        x = synth_block(rsx, torch, nc, sig, c0, min(buf.shape[0], n - c0), buf)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); plain.add(x); torch.cuda.synchronize(); t_plain += time.perf_counter() - t0
        t0 = time.perf_counter(); pt.add(x); torch.cuda.synchronize(); t_pt += time.perf_counter() - t0
        flat.add(x)
    del buf
    emit(case=f"{name}: add", plain_vectors_per_s=round(n / t_plain), through_transform_vectors_per_s=round(n / t_pt),
         plain_s=round(t_plain, 2), through_transform_s=round(t_pt, 2))
    plain.nprobe = pt.index.nprobe = args.nprobe
    Q = torch.empty((nq * 4, D), dtype=torch.float16, device="cuda:0")
    rsx.synth_queries(D, nc, SC, SX, sig, n, SQ, sigq, 0, Q.shape[0], out=Q)
    Qr = opq.apply(Q)
    # the two forms alternate batch by batch inside one loop
    for q0 in (0, nq):
        pt.search(Q[q0:q0 + nq], k); pt.index.search(Qr[q0:q0 + nq], k)
    t_a = t_b = 0.0
    for s in range(args.steps):
        q0 = (s % 4) * nq
        torch.cuda.synchronize(); t0 = time.perf_counter(); pt.search(Q[q0:q0 + nq], k); torch.cuda.synchronize(); t_a += time.perf_counter() - t0
        t0 = time.perf_counter(); pt.index.search(Qr[q0:q0 + nq], k); torch.cuda.synchronize(); t_b += time.perf_counter() - t0
    Da, Ia = pt.search(Q[:nq], k)
    Db, Ib = pt.index.search(Qr[:nq], k)
    emit(case=f"{name}: search, batch {nq}, k {k}", through_transform_ms=round(t_a / args.steps * 1e3, 4),
         pre_rotated_queries_ms=round(t_b / args.steps * 1e3, 4), added_ms=round((t_a - t_b) / args.steps * 1e3, 4), steps=args.steps,
         results_equal=bool(torch.equal(Ia, Ib) and torch.equal(Da, Db)))
    gt = flat.search(Q[:nq], k)[1].cpu().numpy()
    recall = lambda I: round(float(np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(I.cpu().numpy(), gt)])), 4)
    emit(case=f"{name}: recall@10 against the exact Flat search, {nq} queries", ivfpq=recall(plain.search(Q[:nq], k)[1]),
         opq_ivfpq=recall(pt.search(Q[:nq], k)[1]), opq_iterations=opq.niter)
    del flat, plain, pt, Q, Qr
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--opq-niter", type=int, default=4)
    ap.add_argument("--mixtures", default="informative,standard")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch, rsx
    assert rsx.get_num_gpus() > 0, "bench_pretransform needs a GPU"
    apply_cases(rsx, torch, args)
    for mixture in [m for m in args.mixtures.split(",") if m]:
        index_cases(rsx, torch, args, mixture)
    if args.out:
        with open(args.out, "w") as f:
            f.write("| case | figures |\n|---|---|\n")
            for r in ROWS:
                f.write(f"| {r['case']} | " + "; ".join(f"{c} = {v}" for c, v in r.items() if c != "case") + " |\n")


if __name__ == "__main__":
    main()
