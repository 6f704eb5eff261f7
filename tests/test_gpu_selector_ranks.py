"""GPU: filtered search through sharded.ShardedSearcher.search with TWO real ranks sharing cuda:0 over gloo (the form of
tests/test_gpu_two_ranks.py).  The selector is over GLOBAL ids: id-range ranks translate it by their id_offset (local_params) and
the packed all-gather re-bases their local ids; list-shard ranks run the two-call form with the selector in the pre-pass (a filtered
search has no threshold pre-pass: every rank contributes "no threshold" to the all-reduce).  The merged result must be the single
index's filtered result, bit for bit."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, ret):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), os.path.join(os.path.dirname(here), "retrieval-scaling_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    import rsx
    from sharded import ShardedSearcher, shard_range
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    d, n, nq, k, nlist, M = 96, 9000, 33, 12, 8, 32
    x = rsx.synth_vectors(d, 16, 77, 5000, 0.5, 0, n)
    x[6100:6104] = x[40]                    # exact score ties across the two shards
    q = rsx.synth_queries(d, 16, 77, 5000, 0.5, n, 31, 0.1, 0, nq)
    q[0] = x[40]
    rng = np.random.default_rng(9)
    sels = {
        "bitmap50": rsx.IDSelectorBitmap(np.packbits(rng.random(n) < 0.5, bitorder="little")),
        "batch": rsx.IDSelectorBatch(np.array([40, 6101, 6103, 17, 8000, 2, 4499, 4500])),
        "not_range": rsx.IDSelectorNot(rsx.IDSelectorRange(1000, 8000)),
        "range_across": rsx.IDSelectorRange(4000, 5000),
    }
    lo, hi = shard_range(n, rank, world)
    ok = {}
    for kind in ("flat", "ivfpq"):
        if kind == "flat":
            full, local = rsx.IndexFlatIP(d), rsx.IndexFlatIP(d)
        else:
            full = rsx.IndexIVFPQ(None, d, nlist, M, 8, rsx.METRIC_INNER_PRODUCT)
            local = rsx.IndexIVFPQ(None, d, nlist, M, 8, rsx.METRIC_INNER_PRODUCT)
            full.train(x[:4000])
            local.set_centroids(full.get_centroids()); local.set_codebooks(full.get_codebooks())
            full.nprobe = local.nprobe = 4
        full.add(x)
        local.add(x[lo:hi])
        searcher = ShardedSearcher(local, id_offset=lo)
        for name, sel in sels.items():
            p = rsx.SearchParameters(sel=sel) if kind == "flat" else rsx.SearchParametersIVF(sel=sel, nprobe=4)
            Dr, Ir = full.search(q, k, params=p)
            D, I = searcher.search(q, k, params=p)                      # numpy: host merge
            ok[f"{kind}_{name}_numpy"] = bool(np.array_equal(I, Ir) and np.array_equal(D, Dr))
            Dt, It = searcher.search(torch.from_numpy(q).cuda(), k, params=p)     # CUDA: pack kernel (id re-base) + merge kernel
            ok[f"{kind}_{name}_cuda"] = bool(np.array_equal(It.cpu().numpy(), Ir) and np.array_equal(Dt.cpu().numpy(), Dr))
        if kind == "ivfpq":
            ls = rsx.IndexIVFPQ(None, d, nlist, M, 8, rsx.METRIC_INNER_PRODUCT)
            ls.set_centroids(full.get_centroids()); ls.set_codebooks(full.get_codebooks())
            ls.set_param("add_list_mod", world); ls.set_param("add_list_rem", rank)
            ls.nprobe = 4
            ls.add(x)
            qd = torch.from_numpy(q).cuda()
            for name, sel in sels.items():
                p = rsx.SearchParametersIVF(sel=sel, nprobe=4)
                Dl, Il = ShardedSearcher(ls, id_offset=0, exchange_thresholds=True).search(qd, k, params=p)
                Dr, Ir = full.search(q, k, params=p)
                ok[f"list_shards_{name}"] = bool(np.array_equal(Il.cpu().numpy(), Ir) and np.array_equal(Dl.cpu().numpy(), Dr))
    ret[rank] = ok
    dist.barrier()
    dist.destroy_process_group()


def test_filtered_search_two_real_ranks(gpu):
    world = 2
    with mp.Manager() as m:
        ret = m.dict()
        mp.spawn(_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
        got = dict(ret)
    assert set(got) == {0, 1}
    for r in (0, 1):
        bad = [key for key, v in got[r].items() if not v]
        assert not bad, (r, bad)
