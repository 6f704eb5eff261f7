"""GPU: the WHOLE bench.py with N > 1 ranks, as a dry run on one GPU (task 3).

`bench.py --gpus N` had only ever executed with world_size 1: the parameter broadcast, the list-shard add stream, the
ShardedSearcher exchange inside the timed loop, the ground-truth all-gather, the elapsed all-reduce and the self-launch under
torch.distributed.run were dead code as far as any run was concerned.  Here N = 2, 4 and 5 ranks share cuda:0
(`--share-gpu`) and exchange over gloo (`--dist-backend gloo`: RCCL refuses two ranks per device; the collectives are the
same calls routed through host memory), for both partitions of the index (`--shard vectors`: the reference's id-range
shards, src/search.py:282-303; `--shard lists`).  Every run must print ONE JSON line from rank 0 with n_gpus == N, the N = 1
run's recall@10, and the N = 1 run's ids and scores of the first timed batch (sha256 over D and I: the merged result of a
sharded index is the single index's, bit for bit — src/search.py:362-367 is the merge it replaces).

At most six processes may hold the GPU at once.  The test process holds it, and so does the torch.distributed.run agent of a
self-launched run: such a run takes at most MAX_RANKS = 4 ranks.  Five ranks run only when started here directly (_run_ranks)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--n", "1600000", "--nlist", "256", "--chunk", "200000", "--steps", "2", "--warmup", "1", "--cpu-queries", "0",
          "--no-configs", "--no-faiss"]
MAX_RANKS = 4


def _run(extra, full=True):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + COMMON + (["--full"] if full else []) + extra,
                       capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, f"bench.py {extra} failed:\n{p.stderr[-3000:]}"
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"expected ONE JSON line from rank 0, got {len(lines)}:\n{p.stdout[-2000:]}"
    return json.loads(lines[0])


def _run_ranks(n, extra, tmp_path):
    """bench.py as n ranks on cuda:0 over gloo, started here with the env:// rendezvous instead of self-launched: no agent
    process, so one more rank fits under the process limit.  Every rank's output goes to a file (no pipe can fill up)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, WORLD_SIZE=str(n), RANK=str(r), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        out, err = open(tmp_path / f"rank{r}.out", "w"), open(tmp_path / f"rank{r}.err", "w")
        procs.append(subprocess.Popen([sys.executable, os.path.join(REPO, "bench.py")] + COMMON + ["--full"] + extra +
                                      ["--gpus", str(n), "--share-gpu", "--dist-backend", "gloo"], stdout=out, stderr=err, env=env))
        out.close(); err.close()
    try:
        codes = [p.wait(timeout=900) for p in procs]
    finally:                # a rank that died leaves the others waiting in the rendezvous: none may outlive the test
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert codes == [0] * n, f"bench.py ranks {extra} exited {codes}:\n{(tmp_path / 'rank0.err').read_text()[-3000:]}"
    lines = [l for r in range(n) for l in (tmp_path / f"rank{r}.out").read_text().splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"expected ONE JSON line from rank 0, got {len(lines)}"
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def single(gpu):
    r = _run([])
    assert r["n_gpus"] == 1 and r["recall_at_10"] is not None
    return r


@pytest.mark.parametrize("ngpu,shard", [(2, "vectors"), (2, "lists"), (MAX_RANKS, "vectors"), (MAX_RANKS, "lists")])
def test_bench_py_with_n_ranks_on_one_gpu(gpu, single, ngpu, shard):
    r = _run(["--gpus", str(ngpu), "--share-gpu", "--dist-backend", "gloo", "--shard", shard])
    assert r["n_gpus"] == ngpu and r["steps"] == 2 and r["warmup"] == 1
    assert r["config"]["dist_backend"] == "gloo"
    assert r["value"] > 0 and r["ms_per_step"] > 0
    assert r["scaling"] == "strong"
    assert r["recall_at_10"] == single["recall_at_10"], (r["recall_at_10"], single["recall_at_10"])
    assert r["recall_low_noise_queries"] == single["recall_low_noise_queries"]
    assert r["first_timed_batch_sha256"] == single["first_timed_batch_sha256"], "merged D / I of the sharded run differ from the single index"
    if shard == "lists":
        assert "inverted lists" in r["config"]["parallelism"]
    else:
        assert r["config"]["vectors_per_gpu"] == 1600000 // ngpu
    st = r["stage_ms_per_step"]      # round 5: the exchange is reported beside the library's stages when world > 1
    assert all(k_ in st for k_ in ("exchange_pack", "exchange_collective", "exchange_merge")), st
    assert st["exchange_collective"] > 0


def test_bench_py_weak_scaling_switch(gpu):
    """--scaling weak: --n is the shard of EVERY rank (fixed N/GPU), the line says so, and the merged result is
    that of a single index of N x n vectors."""
    r2 = _run(["--gpus", "2", "--share-gpu", "--dist-backend", "gloo", "--scaling", "weak", "--n", "800000"])
    assert r2["n_gpus"] == 2 and r2["scaling"] == "weak"
    assert r2["config"]["vectors_per_gpu"] == 800000 and r2["config"]["workload"].startswith("1600000x")
    r1 = _run([])                                     # the 1.6M-vector single index of COMMON
    assert r2["first_timed_batch_sha256"] == r1["first_timed_batch_sha256"]


def test_five_ranks_at_the_reference_default_k(gpu, tmp_path):
    """k = 4096 (the reference backends' default, src/indicies/flat.py:138) on 5 ranks: 20480 keys per query reach the merge, more
    than one launch holds (16384), so it runs in rounds of pairs, one of them a lone block (round 4 refused nshards * k > 16384).
    Same ids and scores as the single index."""
    extra = ["--k", "4096", "--batch", "64", "--no-recall"]
    r1 = _run(extra)
    r5 = _run_ranks(5, extra, tmp_path)
    assert r5["n_gpus"] == 5 and r5["first_timed_batch_sha256"] == r1["first_timed_batch_sha256"]


def test_dump_outputs_is_the_timed_result(gpu, single, tmp_path):
    """--dump-outputs writes what the last timed step returned: with one timed step that is the first timed batch, whose
    sha256 over D and I the line reports; the same arguments dump the same arrays every run."""
    import hashlib
    import numpy as np
    r = _run(["--steps", "1", "--dump-outputs", str(tmp_path / "one")])
    assert r["steps"] == 1 and r["first_timed_batch_sha256"] == single["first_timed_batch_sha256"]
    D = np.load(tmp_path / "one" / "scores.npy")
    I = np.load(tmp_path / "one" / "ids.npy")
    assert D.dtype == np.float32 and D.shape == (1024, 10) and I.dtype == np.float64 and I.shape == (1024, 10)
    assert hashlib.sha256(D.tobytes() + I.astype(np.int64).tobytes()).hexdigest() == r["first_timed_batch_sha256"]
    _run(["--steps", "1", "--dump-outputs", str(tmp_path / "again")])
    for f in ("scores.npy", "ids.npy", "rows.npy"):
        assert np.array_equal(np.load(tmp_path / "one" / f), np.load(tmp_path / "again" / f)), f


HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config", "settle_batches"}


@pytest.mark.parametrize("ngpu", [1, 2])
def test_plain_run_prints_the_headline_of_the_same_steps(gpu, single, ngpu, tmp_path):
    """Without --full the line holds the headline keys only, each meaning what it means in a --full line, and the last timed
    step returns what it returns there: at --steps 1 the first timed batch, whose sha256 the --full line reports."""
    import hashlib
    import numpy as np
    extra = ["--steps", "1", "--dump-outputs", str(tmp_path / "plain")]
    if ngpu > 1:
        extra += ["--gpus", str(ngpu), "--share-gpu", "--dist-backend", "gloo"]
    r = _run(extra, full=False)
    assert set(r) == HEADLINE, sorted(set(r) ^ HEADLINE)
    assert r["n_gpus"] == ngpu and r["steps"] == 1 and r["warmup"] == 1
    for key in ("metric", "unit", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "settle_batches"):
        assert r[key] == single[key], key
    assert r["config"]["workload"] == single["config"]["workload"]
    assert abs(r["value"] - 1024 / (r["ms_per_step"] * 1e-3)) / r["value"] < 0.01
    D = np.load(tmp_path / "plain" / "scores.npy")
    I = np.load(tmp_path / "plain" / "ids.npy")
    assert hashlib.sha256(D.tobytes() + I.astype(np.int64).tobytes()).hexdigest() == single["first_timed_batch_sha256"]
