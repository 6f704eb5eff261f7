"""CPU: `python bench.py --gpus N` without a launcher must start N ranks by itself (it used to die on
`assert world == args.gpus`).  There is no GPU here, so each rank stops at the "needs a GPU" assertion — which proves the
ranks were started with WORLD_SIZE = N."""
import os
import subprocess
import sys

from conftest import REPO


def test_bench_self_launches_its_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["CUDA_VISIBLE_DEVICES"] = ""          # also on a GPU box: this test is about the launch, not the bench
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--n", "1000"],
                       env=env, capture_output=True, text=True, timeout=600)
    err = r.stderr
    assert r.returncode != 0
    assert "self-launch:" in err and "--nproc-per-node=2" in err
    assert "launch with torch.distributed.run" not in err            # the old failure
    assert err.count("bench.py needs a GPU") >= 2                     # both ranks got as far as the device check


def test_committed_bench_line_keeps_the_contract():
    """The newest full bench line under profiles/ (the driver's `python bench.py` on a GPU box, copied there by the evidence pass)
    carries every key of the bench contract, a roofline whose fraction is achieved / peak, and a CPU baseline that says what it
    is.  bench.py cannot run without a GPU: this guards the line's SHAPE between GPU sessions.  "Newest" is the first bench line
    profiles/INDEX.md lists (newest round first): file times say nothing in a fresh checkout."""
    import json
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = re.findall(r"`(r\w+_bench_ivfpq100M\.json)`", open(os.path.join(root, "profiles", "INDEX.md")).read())
    assert names, "profiles/INDEX.md lists no bench line"
    newest = os.path.join(root, "profiles", names[0])
    assert os.path.exists(newest), f"profiles/INDEX.md lists {names[0]}, which is not committed"
    lines = [l for l in open(newest) if l.startswith("{")]
    assert len(lines) == 1, "the bench prints ONE JSON line"
    j = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "cpu_baseline"):
        assert key in j, key
    assert j["unit"] == "queries/s" and j["higher_is_better"] is True and j["n_gpus"] == 1 and j["data"] == "synthetic"
    assert "workload" in j["config"] and "model" not in j["config"]
    assert abs(j["value"] - 1024 / (j["ms_per_step"] * 1e-3)) / j["value"] < 0.01, "value = queries of a step / time of a step (batch 1024)"
    r = j["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = j["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in c, key
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1
    # round 5: the MFMA-busy counter rides with the traffic stamp, and the same operating point is reported on four other distributions
    assert "mfma_busy" in r and "lds" in r
    od = j.get("other_distributions")
    assert od and set(od) >= {"hot_lists", "hot_probe_sets", "informative", "norm_skew"}, od and list(od)
    for name, leg in od.items():
        assert "error" not in leg, (name, leg.get("error"))
        assert leg["exact_fallback_queries_per_step"] == 0 and leg["oracle_parity_ids_and_scores"] is True, name
        assert leg["ms_per_step"] < 2 * j["ms_per_step"], (name, leg["ms_per_step"])       # no distribution slower than 2x the headline
    assert od["informative"]["recall_by_nprobe"]["nprobe32"]["recall_at_10"] > od["informative"]["recall_by_nprobe"]["nprobe1"]["recall_at_10"]


def test_bench_refuses_zero_timed_steps():
    """--steps is the number of timed steps: zero of them has no time and no last step to report."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, r.stderr


def test_bench_refuses_ab_without_full():
    """--ab times other kernels after the timed steps, which only a --full run goes on to."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--ab"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "needs --full" in r.stderr, r.stderr


def test_dump_outputs_writes_the_step_result(tmp_path, monkeypatch):
    """bench.py --dump-outputs: scores as float32, ids as float64, every query row of a small result; a result over the byte
    cap keeps the same seeded sample of rows every time, under the cap."""
    import numpy as np
    import bench
    rng = np.random.default_rng(3)
    D = rng.standard_normal((1024, 10)).astype(np.float32)
    I = rng.integers(-1, 10 ** 11, size=(1024, 10), dtype=np.int64)
    bench.dump_outputs(str(tmp_path / "all"), D, I)
    s, i, rows = (np.load(tmp_path / "all" / f) for f in ("scores.npy", "ids.npy", "rows.npy"))
    assert s.dtype == np.float32 and i.dtype == np.float64 and rows.dtype == np.float64
    assert np.array_equal(s, D) and np.array_equal(i.astype(np.int64), I) and np.array_equal(rows, np.arange(1024))
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 << 10)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), D, I)
    ra = np.load(tmp_path / "a" / "rows.npy").astype(np.int64)
    assert 0 < len(ra) < 1024 and np.array_equal(ra, np.unique(ra))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in ("scores.npy", "ids.npy", "rows.npy")) <= 64 << 10
    for f in ("scores.npy", "ids.npy", "rows.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    assert np.array_equal(np.load(tmp_path / "a" / "scores.npy"), D[ra])
    assert np.array_equal(np.load(tmp_path / "a" / "ids.npy").astype(np.int64), I[ra])
