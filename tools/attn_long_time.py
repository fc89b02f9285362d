"""Forward + backward time of attention_bnhd on the streaming kernels (csrc/attention_long.hip)
against F.scaled_dot_product_attention on the same bf16 inputs, at the c5 attention shapes:
(B H, N, p) = (512, 499, 0.1) HuBERT-large on 10 s, (512, 1374, 0) DINOv2-L/14 at 518 px, and
(512, 321, 0), the first length past the whole-sequence kernels.

Both run in one process, alternating round by round after a warm-up of each (code objects loaded,
PyTorch's kernel choice made); each round times ITERS forward + backward passes with HIP events.
Reported per shape: the median over the rounds, the run-to-run spread (max - min) / median of each
side, and the ratio of the medians. DESIGN.md section 5 holds the rule that reads these numbers
(attention.LONG_ROUTE). --shapes times other (B, H, N, p), the short family's included (N <= 320 runs
csrc/attention.hip); run under TRIAD_LIB_VARIANT it times another build of the library.

    python tools/attn_long_time.py [--rounds 9] [--iters 10] [--shapes 32x16x261x0,32x16x199x0.1]
        > profiles/attn_long_time.log
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from triad_amd import attention as A  # noqa: E402

SHAPES = ((32, 16, 499, 0.1), (32, 16, 1374, 0.0), (32, 16, 321, 0.0))


def _ours(q, k, v, do, p):
    A.attention_bnhd(q, k, v, 0.125, dropout=p).backward(do)


def _torch(q, k, v, do, p):
    # (B, H, N, 64) views of the same (B, N, H, 64) storage, as attention.sdpa's callers hold them
    o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), dropout_p=p,
                                       scale=0.125)
    o.backward(do.transpose(1, 2))


def _time(fn, args, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(*args)
        for t in args[:3]:
            t.grad = None
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _shapes(text):
    return tuple((int(b), int(h), int(n), float(p)) for b, h, n, p in (s.split("x") for s in text.split(",")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", type=_shapes, default=SHAPES, help="BxHxNxp,... (default: the c5 shapes)")
    a = ap.parse_args()
    torch.manual_seed(0)
    print(f"device {torch.cuda.get_device_name(0)}; LONG_ROUTE {A.LONG_ROUTE}; rounds {a.rounds} x iters {a.iters}, "
          "ms per forward + backward")
    for B, H, N, p in a.shapes:
        q, k, v = (torch.randn(B, N, H, 64, device="cuda").mul_(1.5).to(torch.bfloat16).requires_grad_(True)
                   for _ in range(3))
        do = torch.randn(B, N, H, 64, device="cuda").to(torch.bfloat16)
        args = (q, k, v, do, p)
        for fn in (_ours, _torch):   # warm-up
            _time(fn, args, 3)
        t = {"hip": [], "torch": []}
        for _ in range(a.rounds):
            t["hip"].append(_time(_ours, args, a.iters))
            t["torch"].append(_time(_torch, args, a.iters))
        med = {n: statistics.median(x) for n, x in t.items()}
        spread = {n: (max(x) - min(x)) / med[n] for n, x in t.items()}
        print(f"B*H {B * H} N {N} p {p}: hip {med['hip']:.3f} ms (spread {100 * spread['hip']:.1f} %), "
              f"torch {med['torch']:.3f} ms (spread {100 * spread['torch']:.1f} %), hip / torch "
              f"{med['hip'] / med['torch']:.3f}")
        print("   hip   rounds:", " ".join(f"{x:.3f}" for x in t["hip"]))
        print("   torch rounds:", " ".join(f"{x:.3f}" for x in t["torch"]))


if __name__ == "__main__":
    main()
