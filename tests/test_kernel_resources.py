"""Register / scratch budgets of the product library's hot kernels, read from the built
code object (no GPU needed).

Round 4 lost 5 % of the headline self-play rate to a change that only added claim-queue
bookkeeping to the persistent tower: the kernel went from 32 to 200 bytes of scratch
per lane and the self-play autotuner started picking the per-layer convs.  This test
pins the scratch (spill) bytes and VGPR counts of the kernels the bench and the train
step spend their time in, so such a regression fails on CPU before it reaches a GPU.
Budgets are the measured values of the product build (round 4).
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "alphazero-gomoku_amd", "libazg_pv.so")
LLVM = "/opt/rocm/lib/llvm/bin"

# (kernel-name regex on the mangled name, max private_segment_fixed_size bytes)
SCRATCH_BUDGET = [
    # persistent eval towers, fp32 MFMA (key 19 = 0): the figures include the stack frame of
    # the never-taken timed-out-wait path (pv_tower.hip tower_timeout, noinline so it adds no
    # spill to the tile body).  Building the fragment addresses per tap removes these spills
    # but measured 5 % slower in the fp32 body (scripts/gpu_r5ab.sh): kept for split-fp16 only
    (r"conv_towerILi128ELi64ELi4ELi1ELi8ELi32E", 32),
    (r"conv_towerILi128ELi64ELi2ELi1ELi4ELi32E", 64),
    # C = 256: the board-keyed halo body (VAR 33) spills ~100 B outside the chunk loop and is
    # still 4 % faster than VAR 32's 32 B
    (r"conv_towerILi256ELi64ELi4ELi1ELi8ELi33E", 112),
    (r"conv_towerILi256ELi64ELi2ELi1ELi4ELi33E", 144),
    # split-fp16 towers (halo_tile VAR 99, the eval default, key 19 / 20; VAR 98 the row-keyed
    # form): 128 VGPRs at 4 waves per SIMD, fragment addresses built per tap (round 5: 96-336 B
    # of spills before); the 8-wave 128x64 tile is the tuned one at >= 224 boards
    (r"conv_towerILi128ELi64ELi4ELi1ELi8ELi99E", 0),
    (r"conv_towerILi256ELi64ELi4ELi1ELi8ELi99E", 16),
    (r"conv_towerILi(128|256)ELi64ELi2ELi1ELi4ELi99E", 80),
    (r"conv_towerILi(128|256)ELi64ELi(2|4)ELi1ELi(4|8)ELi98E", 16),
    # h3_tile towers (VAR 355, shape 12: 4 waves of 64x64 at 256 VGPRs): spills outside the
    # chunk loop only (tower claim / epilogue)
    (r"conv_towerILi128ELi128ELi2ELi2ELi4ELi355E", 176),
    (r"conv_towerILi256ELi128ELi2ELi2ELi4ELi355E", 272),
    (r"conv3x3_haloILi(128|256)ELi64ELi(2|4)ELi1ELi(4|8)ELi[01]ELi99E", 0),
    (r"conv_towerILi64ELi64E", 0),
    (r"conv_towerILi128ELi128ELi4ELi1ELi16E", 48),
    # train convs at C <= 128 (the 6x128 train step) and the weight grad
    (r"conv3x3_trainILi(64|128)E", 0),
    (r"conv3x3_wgrad_natILi", 0),
    (r"conv3x3_wgrad_nat2ILi", 0),
    (r"wgrad_reduce_kernel", 0),
    (r"wgrad_reduce_mfma_kernel", 0),
    (r"stem_mfma", 0),
    # board-resident towers (round 6): spills in the per-board staging and the epilogue only
    # (the K loops are scratch-free, checked in the ISA); the 16x16x32 one is the eval default
    # (and projects the heads' features from LDS after its last conv)
    (r"board16_towerILi0ELb0E", 120),
    # its small-batch split form (three 8-wave workgroups per board, two waves per SIMD)
    (r"board16_towerILi0ELb1E", 0),
    (r"board_towerILi0E", 196),
]


def _kernels():
    if not os.path.exists(LIB):
        pytest.skip("libazg_pv.so not built (run __graft_entry__.build())")
    objcopy = shutil.which("objcopy")
    bundler = os.path.join(LLVM, "clang-offload-bundler")
    readelf = os.path.join(LLVM, "llvm-readelf")
    if not objcopy or not os.path.exists(bundler) or not os.path.exists(readelf):
        pytest.skip("objcopy / clang-offload-bundler / llvm-readelf not available")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fb.bin"), os.path.join(d, "co.elf")
        subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fb}", LIB, os.path.join(d, "x.so")], check=True,
                       capture_output=True)
        # one offload bundle per translation unit, concatenated (4 KiB aligned)
        raw = open(fb, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(re.escape(magic), raw)]
        notes = ""
        for i, st in enumerate(starts):
            part = os.path.join(d, f"b{i}.bin")
            with open(part, "wb") as f:
                f.write(raw[st:starts[i + 1] if i + 1 < len(starts) else len(raw)])
            # the budgets are gfx950's (the Makefile's ARCH may name another target):
            # take the bundle's gfx950 entry, skip when the library has none
            ids = subprocess.run([bundler, "--list", "--type=o", f"--input={part}"], capture_output=True,
                                 text=True).stdout.split()
            tgt = next((t for t in ids if t.endswith("gfx950") or "gfx950:" in t), None)
            if tgt is None:
                pytest.skip(f"library built without a gfx950 code object (bundle targets: {ids})")
            subprocess.run([bundler, "--unbundle", "--type=o", f"--input={part}", f"--targets={tgt}",
                            f"--output={co}"], check=True, capture_output=True)
            notes += subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    name = None
    for line in notes.splitlines():
        m = re.match(r"\s*\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
            out.setdefault(name, {})
            continue
        m = re.match(r"\s*\.(private_segment_fixed_size|vgpr_count|agpr_count|vgpr_spill_count):\s+(\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def test_hot_kernels_within_scratch_budget():
    ks = _kernels()
    assert ks, "no kernels found in the code object"
    bad, seen = [], set()
    for pat, budget in SCRATCH_BUDGET:
        hits = [n for n in ks if re.search(pat, n)]
        assert hits, f"no kernel matches {pat}"
        seen.add(pat)
        for n in hits:
            s = ks[n].get("private_segment_fixed_size", 0)
            if s > budget:
                bad.append((n, s, budget))
    assert not bad, "kernels above their scratch budget (spills): " + "; ".join(
        f"{n}: {s} B > {b} B" for n, s, b in bad)


def test_hot_kernels_fit_two_workgroups_per_cu():
    """The 8-wave tower / train tiles run two workgroups per CU: <= 128 VGPRs (+AGPRs)."""
    ks = _kernels()
    for n, v in ks.items():
        if re.search(r"conv_towerILi(128|256)ELi64ELi4ELi1ELi8E|conv3x3_trainILi(64|128)E", n):
            total = v.get("vgpr_count", 0) + v.get("agpr_count", 0)
            assert total <= 128, (n, total)


def test_board_towers_occupancy():
    """board16_tower: 12 waves at <= 168 VGPRs (3 waves per SIMD, one workgroup per CU);
    board_tower: 16 waves at <= 128."""
    ks = _kernels()
    for pat, cap in ((r"board16_towerILi0ELb0E", 168), (r"board_towerILi0E", 128)):
        hits = [n for n in ks if re.search(pat, n)]
        assert hits, pat
        for n in hits:
            total = ks[n].get("vgpr_count", 0) + ks[n].get("agpr_count", 0)
            assert total <= cap, (n, total)
