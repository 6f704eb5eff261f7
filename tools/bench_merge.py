#!/usr/bin/env python3
"""merge_from measurement: joining piece indexes on one GPU, next to the routes a user had before.

Cases (synthetic data as in bench.py; every piece is filled with its own slice of the rows, sequential ids, then merged into the
first piece with add_id = the running ntotal):
  * IVF-PQ n x 768, M = 96, sliced layout, as 2 and as 8 pieces; 2 pieces again with reserve_lists on the destination (no re-layout);
  * IVF-Flat 20M as 2 pieces;
  * IVF-Flat 100M as 2 pieces with exact reservations on both (without them the index does not fit twice).
Per case: wall time of the merges, its split into the copy (rsx_get_timing "merge_copy_ms") and the rest (re-layout, directory
uploads), payload bytes moved per second, peak device memory in use (sampled with hipMemGetInfo from a second thread).
Beside them, in the same process: the re-layout's own copy (launch_copy_lists, timed through an exact reserve_lists that grows
every list of a full index), `add` of the raw vectors into one index (device-resident fp16 rows: no host traffic counted), and
the get_list -> add_list round trip through the host over a sample of lists (extrapolated to the whole index by bytes).
One JSON line per measurement on stdout; --out also writes the table as markdown.

  python tools/bench_merge.py [--n-ivfpq 100000000] [--n-ivfflat-small 20000000] [--n-ivfflat 100000000] [--out profiles/merge_speed.md]
"""
import argparse, json, os, sys, threading, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "retrieval-scaling_amd")); sys.path.insert(0, REPO)
import numpy as np

D, NC, SC, SX = 768, 4096, 1234, 10000
CH = 1_000_000
ROWS = []


def emit(rec):
    ROWS.append(rec)
    print(json.dumps(rec), flush=True)


class PeakMem:
    """device memory in use, sampled every few milliseconds while the block runs"""
    def __init__(self, torch):
        self.torch, self.peak, self.stop = torch, 0, False

    def _run(self):
        while not self.stop:
            free, total = self.torch.cuda.mem_get_info(0)
            self.peak = max(self.peak, total - free)
            time.sleep(0.003)

    def __enter__(self):
        self.th = threading.Thread(target=self._run, daemon=True)
        self.th.start()
        return self

    def __exit__(self, *a):
        self.stop = True
        self.th.join()


def fill(rsx, torch, ix, lo, hi, buf):
    """rows lo .. hi - 1 of the synthetic set; returns the seconds spent inside add alone"""
    t_add = 0.0
    for c0 in range(lo, hi, CH):
        nb = min(CH, hi - c0)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, c0, nb, out=buf[:nb])
        torch.cuda.synchronize(); t0 = time.perf_counter()
        ix.add(buf[:nb])
        t_add += time.perf_counter() - t0
    return t_add


def train(rsx, torch, ix, n, nlist):
    nt = min(n, 256 * nlist)
    xt = torch.empty((nt, D), dtype=torch.float16, device=torch.device("cuda", 0))
    stride = max(1, n // nt)
    for b in range(0, nt, 4096):
        nb = min(4096, nt - b)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, (b * stride) % max(1, n - nb), nb, out=xt[b:b + nb])
    ix.train(xt)
    del xt


def list_counts(rsx, torch, ix, lo, hi, nlist, buf):
    counts = np.zeros(nlist, np.int64)
    for c0 in range(lo, hi, CH):
        nb = min(CH, hi - c0)
        rsx.synth_vectors(D, NC, SC, SX, 0.5, c0, nb, out=buf[:nb])
        counts += np.bincount(np.asarray(ix.assign(buf[:nb])).reshape(-1), minlength=nlist)
    return counts


def merge_case(rsx, torch, name, make, n, pieces, row_bytes, buf, reserve=None, reserve_src=False, nlist=0):
    """make() -> a trained empty index.  reserve: None, or "dst" = reserve_lists(final sizes) on the destination first."""
    cuts = [n * p // pieces for p in range(pieces + 1)]
    parts = []
    for p in range(pieces):
        ix = make()
        if p == 0 and reserve == "dst":
            ix.reserve_lists(list_counts(rsx, torch, ix, 0, n, nlist, buf))
        elif reserve_src:
            ix.reserve_lists(list_counts(rsx, torch, ix, cuts[p], cuts[p + 1], nlist, buf))
        fill(rsx, torch, ix, cuts[p], cuts[p + 1], buf)
        parts.append(ix)
    dst = parts[0]
    torch.cuda.synchronize()
    with PeakMem(torch) as pm:
        t0 = time.perf_counter()
        for src in parts[1:]:
            dst.merge_from(src, dst.ntotal)
        wall = time.perf_counter() - t0
    assert dst.ntotal == n and all(s.ntotal == 0 for s in parts[1:])
    moved = n - cuts[1]
    copy_ms = dst.get_timing("merge_copy_ms")
    emit({"case": name, "pieces": pieces, "reserved": reserve or ("both" if reserve_src else "no"), "rows_moved": moved, "wall_ms": round(wall * 1e3, 1),
          "copy_ms": round(copy_ms, 1), "relayout_and_rest_ms": round(wall * 1e3 - copy_ms, 1), "relayouts": int(dst.get_timing("merge_relayouts")),
          "payload_GB": round(moved * row_bytes / 1e9, 3), "copy_GBps": round(moved * row_bytes / 1e6 / max(copy_ms, 1e-3), 1),
          "merge_GBps": round(moved * row_bytes / 1e9 / wall, 1), "peak_device_GB": round(pm.peak / 1e9, 1)})
    del parts[1:]
    return dst


def relayout_rate(torch, name, ix, row_bytes):
    """launch_copy_lists over the whole index: an exact reservation above every list capacity (the time includes allocating and clearing it)"""
    sizes = ix.list_sizes()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    ix.reserve_lists(2 * sizes + 2048)      # (above every capacity the amortised growth can have left: every list moves)
    ms = (time.perf_counter() - t0) * 1e3
    emit({"case": name, "route": "re-layout (allocation, clearing, launch_copy_lists, directory)", "rows_moved": int(sizes.sum()), "wall_ms": round(ms, 1),
          "GBps": round(int(sizes.sum()) * row_bytes / 1e6 / ms, 1)})


def host_round_trip(rsx, name, full, make, row_bytes, nsample):
    """get_list -> add_list of the first nsample lists through host memory, extrapolated by bytes"""
    dst = make()
    sizes = full.list_sizes()
    t0 = time.perf_counter()
    rows = 0
    for l in range(min(nsample, len(sizes))):
        payload, ids = full.get_list(l)
        if len(ids):
            dst.add_list(l, payload, ids)
        rows += len(ids)
    s = time.perf_counter() - t0
    emit({"case": name, "route": "get_list -> add_list through the host", "lists_sampled": min(nsample, len(sizes)), "rows": rows, "wall_ms": round(s * 1e3, 1),
          "GBps": round(rows * row_bytes / 1e9 / s, 2), "extrapolated_whole_index_s": round(s * int(sizes.sum()) / max(rows, 1), 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ivfpq", type=int, default=100_000_000)
    ap.add_argument("--n-ivfflat-small", type=int, default=20_000_000)
    ap.add_argument("--n-ivfflat", type=int, default=100_000_000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--sample-lists", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch, rsx
    buf = torch.empty((CH, D), dtype=torch.float16, device=torch.device("cuda", 0))
    nlist = args.nlist
    if args.n_ivfpq > 0:
        n, rb = args.n_ivfpq, args.m + 8
        trained = {}

        def make_pq():
            ix = rsx.IndexIVFPQ(rsx.IndexFlatIP(D), D, nlist, args.m, 8, rsx.METRIC_INNER_PRODUCT, device=0)
            ix.set_param("pq_layout", 2.0)
            if not trained:
                train(rsx, torch, ix, n, nlist)
                trained["c"], trained["b"] = ix.get_centroids(), ix.get_codebooks()
            else:
                ix.set_centroids(trained["c"]); ix.set_codebooks(trained["b"])
            return ix
        name = f"ivfpq {n}x{D} M={args.m} nlist={nlist} sliced"
        one = make_pq()
        t_add = fill(rsx, torch, one, 0, n, buf)
        emit({"case": name, "route": "add of the raw vectors into one index (device-resident fp16 rows)", "rows": n, "add_s": round(t_add, 2)})
        host_round_trip(rsx, name, one, make_pq, rb, args.sample_lists)
        relayout_rate(torch, name, one, rb)
        del one
        for pieces, reserve in ((2, None), (8, None), (2, "dst")):
            try:
                d = merge_case(rsx, torch, name, make_pq, n, pieces, rb, buf, reserve=reserve, nlist=nlist)
                del d
            except RuntimeError as e:
                emit({"case": name, "pieces": pieces, "error": str(e)[:300]})
    for n, reserve_both in ((args.n_ivfflat_small, False), (args.n_ivfflat, True)):
        if n <= 0:
            continue
        rb = D * 2 + 8
        cen = {}

        def make_flat():
            ix = rsx.IndexIVFFlat(rsx.IndexFlatIP(D), D, nlist, rsx.METRIC_INNER_PRODUCT, device=0)
            if not cen:
                train(rsx, torch, ix, n, nlist)
                cen["c"] = ix.get_centroids()
            else:
                ix.set_centroids(cen["c"])
            return ix
        name = f"ivfflat {n}x{D} nlist={nlist} fp16"
        try:
            if not reserve_both:
                one = make_flat()
                t_add = fill(rsx, torch, one, 0, n, buf)
                emit({"case": name, "route": "add of the raw vectors into one index (device-resident fp16 rows)", "rows": n, "add_s": round(t_add, 2)})
                host_round_trip(rsx, name, one, make_flat, rb, args.sample_lists)
                relayout_rate(torch, name, one, rb)
                del one
                d = merge_case(rsx, torch, name, make_flat, n, 2, rb, buf, nlist=nlist)
            else:
                d = merge_case(rsx, torch, name, make_flat, n, 2, rb, buf, reserve="dst", reserve_src=True, nlist=nlist)
            del d
        except RuntimeError as e:
            emit({"case": name, "error": str(e)[:300]})
    if args.out:
        keys = []
        for r in ROWS:
            keys += [k for k in r if k not in keys]
        with open(args.out, "w") as f:
            f.write("| " + " | ".join(keys) + " |\n|" + "---|" * len(keys) + "\n")
            for r in ROWS:
                f.write("| " + " | ".join(str(r.get(k, "")) for k in keys) + " |\n")


if __name__ == "__main__":
    main()
