"""Forward + backward of the AV contrastive head in both precisions (ops.contrastive_head,
precision="bf16" against precision="fp32") at the c3 shape (B = 256, Na = 199, Nv = 211).

HIP-event time of every forward + backward after warm-up, the two precisions alternated in one
process on the same seeded fp32 features (the bf16 path gets them as bf16 tensors, as autocast
hands them over). Prints one JSON line per precision (min / median / max ms over the timed
iterations) and one with the ratio of the medians, and writes them to
profiles/head_fp32_bench.json. By MFMA count the fp32 mode does 12 GEMM units (three-term S,
three-term recomputed S, three dQ, three dK) against 3: a ratio of at least 4 is expected.

    python tools/head_fp32_bench.py [--iters 50] [--warmup 3] [--B 256 --Na 199 --Nv 211] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from triad_amd import ops  # noqa: E402


def step(q, k, t, precision):
    q.grad = k.grad = t.grad = None
    losses, _, _ = ops.contrastive_head(ops.AV, q, k, t, precision=precision)
    losses[0].backward()
    return losses[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--Na", type=int, default=199)
    ap.add_argument("--Nv", type=int, default=211)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_fp32_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_fp32_bench needs a HIP device: there is no CPU timing of this head")
    gen = torch.Generator(device="cuda").manual_seed(0)
    q32 = torch.randn(a.B, a.Na, 512, device="cuda", generator=gen) * 0.58
    k32 = torch.randn(a.B, a.Nv, 512, device="cuda", generator=gen) * 0.58
    feats = {"fp32": (q32.requires_grad_(True), k32.requires_grad_(True)),
             "bf16": (q32.detach().to(torch.bfloat16).requires_grad_(True),
                      k32.detach().to(torch.bfloat16).requires_grad_(True))}
    t = torch.tensor(1.5, device="cuda", requires_grad=True)
    order = ("bf16", "fp32")
    loss = {}
    for _ in range(a.warmup):
        for p in order:
            loss[p] = float(step(*feats[p], t, p).detach())
    torch.cuda.synchronize()
    ms = {p: [] for p in order}
    for _ in range(a.iters):
        for p in order:   # alternated: both see the same clocks and neighbours
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(*feats[p], t, p)
            e1.record()
            e1.synchronize()
            ms[p].append(e0.elapsed_time(e1))
    g = ops.Geometry(a.B, a.Na, a.B, a.Nv)
    flops = 3 * 2.0 * g.R * g.Bk * g.Nk_eff * 512   # S, dQ, dK of the algorithm (one GEMM unit each)
    rows = []
    for p in order:
        v = sorted(ms[p])
        rows.append({"tool": "head_fp32_bench", "precision": p, "shape": [a.B, a.Na, a.Nv], "iters": a.iters,
                     "warmup": a.warmup, "ms_min": round(v[0], 3), "ms_median": round(statistics.median(v), 3),
                     "ms_max": round(v[-1], 3), "algorithmic_tflops_at_median": round(flops / statistics.median(v) / 1e9, 1),
                     "loss": loss[p]})
    rows.append({"tool": "head_fp32_bench", "fp32_over_bf16_median": round(rows[1]["ms_median"] / rows[0]["ms_median"], 2),
                 "fp32_over_bf16_min": round(rows[1]["ms_min"] / rows[0]["ms_min"], 2), "expected_by_mfma_count": 4.0,
                 "fp32_chunks": ops.split_num_chunks(g, ops._default_budget(q32.device))})
    for r in rows:
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
