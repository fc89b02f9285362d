"""A/B of the eight-wave 256 x 256 GEMM (gemm_w8_kernel, tile form 4) between two builds of the
library loaded into one process: the tree's and --other PATH (e.g. the parent commit's, built
from a checkout of it). Per shape: seeded N(0, 1) bf16 operands (zeros read high), warm-up, then
the two libraries alternated round by round (9 rounds x 20 calls between HIP events); prints both
medians of the per-round means, each side's spread (max - min) / median, the ratio other / tree
and whether the two outputs are bit-equal. Per instantiation: sum(launches x time) round by round,
its median and spread on both sides, and the verdict of the rule "the new loop stays only if the
sum is lower by more than the larger of the two spreads".

Default shapes: the c3 launches of each instantiation -- the ViT / HuBERT encoder projections at
M = 66,816 and 50,944 tokens (12 layers each: weight 12), the conv stack's products
(frontend._gemm_rows; overlapping A rows, lda = 1024 < K = 1536), and the split-K weight gradients
with the split counts of linear._form_splits / frontend._conv_dw_plan.

usage: python tools/gemm_w8_ab.py --other PATH [--rounds 9] [--calls 20] [--only tt|tn|nn]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from triad_amd import _lib as L  # noqa: E402
from triad_amd import frontend, linear  # noqa: E402

BF = torch.bfloat16
TOKENS = (66816, 50944)


def shapes():
    """(instantiation, label, launches per step, dict of the call)."""
    out = []
    for M in TOKENS:
        for N, K in ((2304, 768), (768, 768), (3072, 768), (768, 3072)):       # forward: x W^T
            out.append(("tt", f"fwd {M}x{N}x{K}", 12, dict(M=M, N=N, K=K, ak=1, bk=1)))
        for N, K in ((768, 2304), (768, 768), (768, 3072), (3072, 768)):       # input gradient: dy W
            out.append(("tn", f"dx {M}x{N}x{K}", 12, dict(M=M, N=N, K=K, ak=1, bk=0)))
        for O, K in ((2304, 768), (768, 768), (3072, 768), (768, 3072)):       # weight gradient: dy^T x
            form, sp = linear._form_splits(M, O, K)
            out.append(("nn", f"dw {O}x{K} over {M} / {sp}", 6, dict(M=O, N=K, K=M, ak=0, bk=0, splits=sp, form=form)))
    # the conv stack (frontend._gemm_rows: layouts (1, 1), b [N][K]; kernel-3 layers read overlapping rows)
    for M, N, K, lda in ((819200, 512, 1536, 1024), (409600, 512, 1536, 1024), (204800, 512, 1536, 1024),
                         (102400, 512, 1024, 1024), (51200, 512, 1024, 1024),
                         (1638400, 512, 512, 512), (819200, 512, 1024, 1024), (102400, 1024, 512, 512)):
        out.append(("tt", f"conv {M}x{N}x{K} lda {lda}", 1, dict(M=M, N=N, K=K, ak=1, bk=1, lda=lda)))
    for M, O, N in ((819200, 512, 1536), (102400, 512, 1024)):
        form, sp = frontend._conv_dw_plan(M, O, N)
        out.append(("nn", f"conv dw {O}x{N} over {M} / {sp}", 1, dict(M=O, N=N, K=M, ak=0, bk=0, splits=sp, form=form)))
    return out


def load(path):
    lib = C.CDLL(path)
    for name in ("triad_gemm_bf16_form", "triad_gemm_bf16_splitk_form"):
        fn = getattr(lib, name)
        fn.argtypes = L.SIGNATURES[name]
        fn.restype = C.c_int
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="path of the other build of libtriad_hip.so")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    libs = {"tree": load(L.DEFAULT_LIB), "other": load(a.other)}
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sums = {}
    for inst, label, launches, s in shapes():
        if a.only and inst != a.only:
            continue
        M, N, K, ak, bk = s["M"], s["N"], s["K"], s["ak"], s["bk"]
        lda = s.get("lda", K if ak else M)
        ldb = K if bk else N
        A = torch.randn((lda * (M - 1) + K) if ak else K * M, device=dev, generator=g).to(BF)
        B = torch.randn(N * K, device=dev, generator=g).to(BF)
        splits = s.get("splits", 0)
        outs = {k: torch.empty(M, N, dtype=BF, device=dev) for k in libs}
        slabs = torch.empty(max(1, splits) * M * N, dtype=torch.float32, device=dev) if splits else None

        def call(k):
            if splits:
                rc = libs[k].triad_gemm_bf16_splitk_form(A.data_ptr(), lda, ak, B.data_ptr(), ldb, bk, M, N, K, splits,
                                                         None, slabs.data_ptr(), outs[k].data_ptr(), 1, s["form"], st)
            else:
                rc = libs[k].triad_gemm_bf16_form(A.data_ptr(), lda, ak, B.data_ptr(), ldb, bk, M, N, K, None,
                                                  outs[k].data_ptr(), N, 1, 4, st)
            assert rc == 0, (label, k, rc)
        for k in libs:
            for _ in range(3):
                call(k)
        torch.cuda.synchronize()
        equal = torch.equal(outs["tree"], outs["other"]) and bool(torch.isfinite(outs["tree"].float()).all())
        times = {k: [] for k in libs}
        for _ in range(a.rounds):
            for k in libs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    call(k)
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.calls * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        spr = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
        tf = 2.0 * M * N * K / med["tree"] * 1e-6
        print(f"{inst} {label:38s} tree {med['tree']:9.1f} us (spread {spr['tree']:.3f})  other {med['other']:9.1f} us "
              f"(spread {spr['other']:.3f})  other/tree {med['other'] / med['tree']:.3f}  {tf:6.0f} TFLOP/s  "
              f"equal {equal}", flush=True)
        t = sums.setdefault(inst, dict(tree=[0.0] * a.rounds, other=[0.0] * a.rounds, equal=True))
        for k in libs:   # the weighted sum round by round: its own median and spread
            t[k] = [x + launches * y for x, y in zip(t[k], times[k])]
        t["equal"] &= equal
        del A, B, outs, slabs
    for inst, t in sums.items():
        med = {k: statistics.median(t[k]) for k in libs}
        spr = {k: (max(t[k]) - min(t[k])) / med[k] for k in libs}
        gain = 1.0 - med["tree"] / med["other"]
        print(f"== {inst}: sum(launches x time) per round, median: tree {med['tree'] / 1e3:.2f} ms (spread "
              f"{spr['tree']:.3f}), other {med['other'] / 1e3:.2f} ms (spread {spr['other']:.3f}), tree lower by "
              f"{gain:.3f}, all equal {t['equal']} -> "
              f"{'tree faster' if gain > max(spr.values()) else 'not faster by more than the spread'}")


if __name__ == "__main__":
    main()
