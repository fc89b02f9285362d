"""The steady loop of gemm_w8_tiles_kernel (csrc/gemm.hip: the pipelined loop of the one-tile kernel
run over the concatenated k loops of a workgroup's tiles, with the tile's output written at the
seam inside the loop), checked on hipcc's own output (hipcc -S for gfx950 with the product flags;
no GPU needed) for all eight instantiations. Counters and barriers only:

1. between the loop's header label and its back branch, seam code included, there is no
   `s_waitcnt vmcnt(0)` and no vmcnt wait that hipcc added (it adds vmcnt(0) at the first use of an
   ordinary load's result while an LDS-DMA is in flight: the reason the seam's bias comes through
   LDS);
2. the loop covers whole k-steps of 32 MFMAs per wave, each with four runs of 2 16-byte LDS-DMA
   instructions (one half-tile per phase) and one hand-written vmcnt(6) after the fourth: the
   schedule of the one-tile kernel, unchanged. (The bias piece is a 4- or 2-byte LDS-DMA, one per
   tile and wave, issued ahead of a k-step's first run: older than everything the wait leaves in
   flight. It is not a stage piece and not counted in the runs.);
3. every MFMA cluster sits between two barriers;
4. every k-step of the loop carries a seam of 128 stores per wave, and there is no barrier between
   a seam's first and last store (the seam adds no barrier: 1 + 8 x stages per wave row);
5. no scratch (.private_segment_fixed_size 0) and .vgpr_count within 256.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "triad_amd", "csrc", "gemm.hip")
NAME = "gemm_w8_tiles_kernel"
FLIGHT, LOADS, HALF_TILES = 3, 2, 4
MFMA_PER_STEP = 32     # per wave: 128 x 64 output of 32 x 32 tiles, four 16-deep steps
STORES_PER_SEAM = 128  # per wave: 128 x 64 outputs / 64 lanes


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import sys
    sys.path.insert(0, ROOT)
    from triad_amd import build
    out = tmp_path_factory.mktemp("isa_w8_tiles") / "gemm.s"
    flags = [f for f in build.FLAGS if f != "-fPIC"]
    subprocess.run([hipcc, *flags, *build.EXTRA.get("gemm.hip", []), "--cuda-device-only", "-S", SRC, "-o", str(out)],
                   check=True, capture_output=True)
    return out.read_text()


@pytest.fixture(scope="module")
def kernels(asm):
    """{symbol: [instruction lines]} of the gemm_w8_tiles_kernel instantiations."""
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
    ks = {s: l for s, l in res.items() if NAME in s}
    assert len(ks) == 8, sorted(ks)   # four layouts x {bf16, fp32}
    return ks


def _span(lines):
    """The loop that holds MFMAs: header label .. its last back branch."""
    best = None
    for hdr in (i for i, l in enumerate(lines) if "Loop Header" in l):
        label = lines[hdr].split(":")[0]
        backs = [i for i, l in enumerate(lines)
                 if i > hdr and re.match(r"s_(cbranch_\w+|branch)\s+" + re.escape(label) + r"$", l)]
        if backs and any(l.startswith("v_mfma") for l in lines[hdr:max(backs)]):
            assert best is None, "more than one MFMA loop"
            best = (hdr, max(backs))
    assert best is not None, "no MFMA loop"
    return best


def _events(lines):
    """('D', n): a run of n 16-byte LDS-DMA instructions; ('W', N) / ('w', N): a hand-written /
    hipcc-added vmcnt(N); ('B', 0): s_barrier; ('M', n): a run of n MFMAs; ('S', n): n stores since
    the last barrier or MFMA."""
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
            continue
        for key, prefix in (("D", "global_load_lds_dwordx4"), ("M", "v_mfma"), ("S", "global_store")):
            if t.startswith(prefix):
                if ev and ev[-1][0] == key:
                    ev[-1] = (key, ev[-1][1] + 1)
                else:
                    ev.append((key, 1))
                break
        else:
            if t.startswith("s_barrier"):
                ev.append(("B", 0))
    return ev


def test_steady_loop_and_seam(kernels):
    for sym, lines in kernels.items():
        hdr, back = _span(lines)
        ev = _events(lines[hdr:back])
        waits = [n for k, n in ev if k in "Ww"]
        assert 0 not in waits, (sym, waits)                                   # 1: nothing drains the DMA
        assert not [n for k, n in ev if k == "w"], (sym, ev)                  # 1: hipcc added no vmcnt wait
        mfma = sum(n for k, n in ev if k == "M")
        assert mfma and mfma % MFMA_PER_STEP == 0, (sym, mfma)
        steps = mfma // MFMA_PER_STEP
        runs = [n for k, n in ev if k == "D"]
        assert runs == [LOADS] * (HALF_TILES * steps), (sym, runs)            # 2
        assert waits == [LOADS * FLIGHT] * steps, (sym, waits)
        seq = [k for k, _ in ev if k in "DW"]
        assert seq == (["D"] * HALF_TILES + ["W"]) * steps, (sym, seq)
        # 3: every MFMA cluster sits between two barriers (stores and waits are not barriers)
        sync = [k for k, _ in ev if k in "MB"]
        for i, k in enumerate(sync):
            if k == "M":
                assert i > 0 and sync[i - 1] == "B" and i + 1 < len(sync) and sync[i + 1] == "B", (sym, i)
        assert sync.count("B") == 8 * steps, (sym, sync.count("B"))           # eight barriers per stage
        # 4: a seam per k-step; between the stores of one seam neither a barrier nor an MFMA
        seams = [n for k, n in ev if k == "S"]
        assert seams == [STORES_PER_SEAM] * steps, (sym, seams)


def test_whole_kernel_seams_have_no_barrier(kernels):
    """Outside the loop too (the rest stages and the drain): stores come in whole seams."""
    for sym, lines in kernels.items():
        seams = [n for k, n in _events(lines) if k == "S"]
        assert seams and set(seams) == {STORES_PER_SEAM}, (sym, seams)


def test_no_scratch_and_registers_within_256(asm):
    found = 0
    for m in re.finditer(r"\.name:\s+(\S*" + NAME + r"\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", asm):
        found += 1
        assert int(m.group(2)) == 0, (m.group(1), "scratch", m.group(2))       # 5
        assert int(m.group(3)) <= 256, (m.group(1), "vgprs", m.group(3))
    assert found == 8, found
