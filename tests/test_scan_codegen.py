"""Conditions of k_pq_scan_sl8's design that only the compiler's output shows (profiles/sl8_block_loop.md): the sub-tile loop holds the
look-ups and no spill traffic.  The kernel sits at the 128-VGPR ceiling of sixteen waves per CU, so one more live register turns into
scratch accesses that share the in-order vmcnt queue with the code prefetch, and hoisted wave-uniform state turns into v_readlane /
v_writelane around every block.  Compiles k_pq_rot.hip for the device only, with the Makefile's flags; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "retrieval-scaling_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")


def _makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", mk, re.M).group(1)
    return re.search(r"^FLAGS = (.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()


def _define(src, name):
    return int(re.search(r"^#define %s (\d+)" % name, src, re.M).group(1))


@pytest.fixture(scope="module")
def sl8(tmp_path_factory):
    """(instructions of the launcher's k_pq_scan_sl8 instantiation, its metadata block, SL8_NB)"""
    src = open(os.path.join(CSRC, "k_pq_rot.hip")).read()
    nb, rd = _define(src, "SL8_NB"), _define(src, "SL8_RD")
    assert "launch_pq_scan_sl8_t<3, SL8_NB, SL8_RD>" in src, "the launcher's instantiation is no longer <3, SL8_NB, SL8_RD>"
    out = str(tmp_path_factory.mktemp("sl8") / "k_pq_rot.s")
    cc = subprocess.run(["hipcc"] + _makefile_flags() + ["--cuda-device-only", "-S", os.path.join(CSRC, "k_pq_rot.hip"), "-o", out],
                        cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, "hipcc failed:\n" + cc.stdout[-4000:]
    asm = open(out).read()
    names = set(re.findall(r"^(_ZN3rsx13k_pq_scan_sl8ILi3ELi%dELi%dEE\w*):" % (nb, rd), asm, re.M))
    assert len(names) == 1, names
    name = names.pop()
    body = asm[asm.index("\n" + name + ":"):]
    body = body[:body.index(".Lfunc_end")]
    ins = []
    for line in body.splitlines():
        line = line.split(";")[0].strip()
        if line and not line.endswith(":") and not line.startswith("."):
            ins.append(line.split()[0])
    meta = [b for b in asm.split("  - .agpr_count")[1:] if re.search(r"\.name:\s+%s\n" % re.escape(name), b)]
    assert len(meta) == 1
    return ins, meta[0], nb


def _meta(block, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))


def test_no_vgpr_spill_and_no_scratch(sl8):
    _, meta, _ = sl8
    assert _meta(meta, "vgpr_spill_count") == 0
    assert _meta(meta, "private_segment_fixed_size") == 0


def test_sgpr_spills_stay_outside_the_loop_and_few(sl8):
    """SGPR spills are tolerable only in the item prologue / epilogue (2 at the time of writing, 105 before the loop was cleaned): the
    loop test below forbids their v_readlane / v_writelane between the MFMAs, this one keeps the count from creeping back."""
    _, meta, _ = sl8
    n = _meta(meta, "sgpr_spill_count")
    print("k_pq_scan_sl8 SGPR spills:", n)
    assert n <= 8


def test_no_spill_traffic_between_the_first_and_the_last_mfma(sl8):
    ins, _, _ = sl8
    at = [i for i, m in enumerate(ins) if m.startswith("v_mfma")]
    loop = ins[at[0]:at[-1] + 1]
    bad = [m for m in loop if m.startswith("scratch_") or m in ("v_readlane_b32", "v_writelane_b32")]
    assert not bad, sorted(set(bad))


def test_one_unrolled_block_body_per_pass_and_block(sl8):
    ins, _, nb = sl8
    assert sum(m.startswith("v_mfma") for m in ins) == 8 * 3 * nb
