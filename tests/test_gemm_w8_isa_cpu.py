"""The pipelined main loop of gemm_w8_kernel (csrc/gemm.hip), checked on hipcc's own output
(hipcc -S for gfx950 with the product flags; no GPU needed), for every gemm_w8_kernel symbol that
runs it (the pipelined loop is the one with s_setprio around its MFMA clusters):

1. between the loop's header label and its back branch there is no `s_waitcnt vmcnt(0)`, neither
   hand-written nor added by hipcc (hipcc adds one before the first ds_read of a k-step when it
   sees a second __shared__ object beside the staging array, or any load it counts), and the loop
   has raw s_barriers;
2. the loop covers whole k-steps of 32 MFMAs per wave, each with four runs of L LDS-DMA
   instructions (one half-tile per phase, L = 2: 16 KB / (512 lanes x 16 B)) and one counted wait
   after the fourth; the wait retires the stage whose last half-tile is the first of those runs
   and leaves the other three in flight, so it must be vmcnt(3 L) -- L is counted from the emitted
   runs, 3 is what the comment above the loop says (GP_FLIGHT);
3. after the loop, the last hand-written wait before the last phase that reads LDS is vmcnt(0),
   with a barrier between the wait and the reads.

Verified by hand: with TRIAD_VMCNT(GP_LOADS * GP_FLIGHT) edited to + 1 or - 1, with GP_FLIGHT = 2
or 4, and with the drain's vmcnt(0) made vmcnt(2), this test fails; with __syncthreads()-style
vmcnt(0) added in the loop it fails on check 1.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "triad_amd", "csrc", "gemm.hip")
FLIGHT = 3          # half-tiles the steady-state wait leaves in flight (the comment above the loop)
HALF_TILES = 4      # per stage: two of A, two of B
MFMA_PER_STEP = 32  # per wave: 128 x 64 output of 32 x 32 tiles, four 16-deep steps


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{symbol: [instruction lines]} of the gemm_w8_kernel instantiations."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import sys
    sys.path.insert(0, ROOT)
    from triad_amd import build
    out = tmp_path_factory.mktemp("isa_w8") / "gemm.s"
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    subprocess.run([hipcc, *flags, *build.EXTRA.get("gemm.hip", []), "--cuda-device-only", "-S", SRC, "-o", str(out)],
                   check=True, capture_output=True)
    asm = out.read_text()
    names = set(re.findall(r"^\s+\.amdhsa_kernel (\S+)", asm, re.M))
    res, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(\S+):", line)
        if m and m.group(1) in names:
            cur = m.group(1)
            res[cur] = []
        elif cur is not None:
            if line.strip().startswith(".Lfunc_end"):
                cur = None
            else:
                res[cur].append(line.strip())
    return {s: l for s, l in res.items() if "gemm_w8_kernel" in s}


def _pipelined(kernels):
    ks = {s: l for s, l in kernels.items() if any(x.startswith("s_setprio") for x in l)}
    assert len(kernels) == 8, sorted(kernels)   # four layouts x {bf16, fp32}
    assert len(ks) == 8, sorted(ks)             # every instantiation runs the pipelined loop
    return ks


def _span(lines):
    hdr = next(i for i, l in enumerate(lines) if "Loop Header" in l)
    label = lines[hdr].split(":")[0]
    back = max(i for i, l in enumerate(lines) if re.match(r"s_(cbranch_\w+|branch)\s+" + re.escape(label) + r"$", l))
    return hdr, back


def _events(lines):
    """('D', n) for a run of n LDS-DMA instructions with no barrier between, ('W', N) for a
    hand-written vmcnt(N), ('w', N) for one hipcc added, 'B' for s_barrier, 'R' for a run of LDS
    reads, 'M' for a run of MFMAs."""
    ev, inside = [], False
    for t in lines:
        if t.startswith(";;#ASMSTART"):
            inside = True
            continue
        if t.startswith(";;#ASMEND"):
            inside = False
            continue
        if not t or t[0] in ";.":
            continue
        m = re.match(r"s_waitcnt\s.*vmcnt\((\d+)\)", t)
        if m:
            ev.append(("W" if inside else "w", int(m.group(1))))
        elif t.startswith("global_load_lds_dwordx4"):
            if ev and ev[-1][0] == "D":
                ev[-1] = ("D", ev[-1][1] + 1)
            else:
                ev.append(("D", 1))
        elif t.startswith("s_barrier"):
            ev.append(("B", 0))
        elif t.startswith("ds_read"):
            if not (ev and ev[-1][0] == "R"):
                ev.append(("R", 0))
        elif t.startswith("v_mfma"):
            if ev and ev[-1][0] == "M":
                ev[-1] = ("M", ev[-1][1] + 1)
            else:
                ev.append(("M", 1))
    return ev


def test_source_says_three_half_tiles_in_flight():
    text = open(SRC).read()
    assert re.search(r"constexpr int GP_FLIGHT = (\d+);", text).group(1) == str(FLIGHT)
    assert "TRIAD_VMCNT(GP_LOADS * GP_FLIGHT)" in text


def test_loop_has_no_drain_and_counted_waits_match(kernels):
    for sym, lines in _pipelined(kernels).items():
        hdr, back = _span(lines)
        ev = _events(lines[hdr:back])
        waits = [n for k, n in ev if k in "Ww"]
        assert 0 not in waits, (sym, waits)                       # 1: nothing drains the DMA
        assert not [n for k, n in ev if k == "w"], (sym, ev)      # hipcc added no vmcnt wait at all
        assert sum(1 for k, _ in ev if k == "B") >= 2, sym
        mfma = sum(n for k, n in ev if k == "M")
        assert mfma and mfma % MFMA_PER_STEP == 0, (sym, mfma)
        steps = mfma // MFMA_PER_STEP
        runs = [n for k, n in ev if k == "D"]
        assert len(runs) == HALF_TILES * steps and len(set(runs)) == 1, (sym, runs)   # 2
        L = runs[0]
        assert L == 2, (sym, L)
        assert len(waits) == steps and set(waits) == {L * FLIGHT}, (sym, waits, L)
        # each counted wait follows the fourth run since the previous one, before that phase's barrier
        seq = [k for k, _ in ev if k in "DW"]
        assert seq == ["D"] * HALF_TILES + ["W"] if steps == 1 else seq == (["D"] * HALF_TILES + ["W"]) * steps, (sym, seq)
        # every MFMA cluster sits between two barriers
        for i, (k, _) in enumerate(ev):
            if k == "M":
                assert ev[i - 1][0] == "B" and (i + 1 == len(ev) or ev[i + 1][0] == "B"), (sym, i)


def test_drain_ends_in_vmcnt0_before_the_last_reads(kernels):
    for sym, lines in _pipelined(kernels).items():
        _, back = _span(lines)
        ev = _events(lines[back + 1:])
        last_read = max(i for i, (k, _) in enumerate(ev) if k == "R")
        # the last k-step: the reads of its three reading phases; go back to the first of them
        before = ev[:last_read]
        wi = max(i for i, (k, _) in enumerate(before) if k == "W")
        assert before[wi][1] == 0, (sym, before[wi])              # 3
        assert any(k == "B" for k, _ in before[wi + 1:]), sym
        # no LDS read between that wait and the barrier after it
        nb = next(i for i in range(wi + 1, len(before)) if before[i][0] == "B")
        assert not any(k == "R" for k, _ in before[wi + 1:nb]), sym
        assert not [n for k, n in ev[wi + 1:last_read] if k == "D"], sym   # nothing issued after the drain
