"""CPU: the IVF-PQ append of merge_from / copy_subset_to (csrc/k_merge.h) emulated on host memory for every ordered pair of code
layouts, every phase of source and destination rows and the tile boundaries of the work items.  The check is a small host program
compiled from the engine's own header with hipcc (no GPU, no kernel launch)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_pq_merge_mapping_on_the_host(tmp_path):
    exe = str(tmp_path / "merge_check")
    src = os.path.join(REPO, "tests", "host", "merge_check.hip")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O2", "-pthread", "-std=c++17", "-Wno-unused-value", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "merge ok: 19 layout pairs" in out.stdout, out.stdout + out.stderr
