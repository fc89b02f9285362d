"""Forward + backward time of the HuBERT-large encoder (HubertEncoderStableLayerNorm, 24 layers, hidden
1024, 16 heads) on the fused pre-LN path (postln._stable_encoder_forward, csrc/postln.hip triad_preln_*)
against the stock transformers loop (`_triad_stock_forward`), on 10 s of audio (499 tokens per clip) at
B = 32 (15 968 rows, the c5 per-rank batch) and B = 8.

Both forwards run in one process on the same module, alternating round by round after a warm-up of each
(two unreported rounds of each per shape: code objects loaded, GEMM choices made, clocks settled). The
encoder is in training mode under bf16 autocast with the model's own dropout (0.1) and LayerDrop (0.1);
torch.manual_seed is reset to the same value before every round, so every round of both sides skips the
same layers. Each round times ITERS forward + backward passes with HIP events. Reported per batch size:
the median over the rounds, the run-to-run spread (max - min) / median of each side, and the ratio of
the medians. DESIGN.md section 4b holds the rule that reads these numbers (postln.STABLE_ROUTE).
--kernels adds one timed pass of the preln kernels alone at the same row count (bytes moved over time).

    python tools/audio_large_time.py [--rounds 9] [--iters 10] [--batches 32,8] [--kernels]
        > profiles/preln_time.log
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from triad_amd import model as Mdl  # noqa: E402
from triad_amd import postln  # noqa: E402

TOKENS = 499     # 10 s at 16 kHz through the conv feature encoder


def _pass(enc, fwd, x, gy):
    enc.forward = fwd
    x.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = enc(x).last_hidden_state
    out.backward(gy)


def _time(enc, fwd, x, gy, iters, seed):
    torch.manual_seed(seed)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        _pass(enc, fwd, x, gy)
    e1.record()
    e1.synchronize()
    enc.zero_grad(set_to_none=True)
    return e0.elapsed_time(e1) / iters


def _event_ms(fn, iters=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _kernels(M, D=1024):
    """The residual pass alone at M rows: triad_preln_fwd (reads res, y; writes res_out, n: 8 B per
    element) and triad_preln_bwd with both gradients (reads dz, dn, z; writes dres, dy: 10 B per element,
    + the partials), called through the C ABI back to back on the same buffers: 131 / 164 MB at 15 968
    rows, past the L2s but inside the 256 MB Infinity Cache, so the rate is not an HBM rate."""
    from triad_amd._lib import call, ptr, stream_ptr
    dev = "cuda"
    res, y, dz, dn = ((torch.randn(M, D, device=dev)).to(torch.bfloat16) for _ in range(4))
    w, b = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    z, n, dres, dy = (torch.empty(M, D, dtype=torch.bfloat16, device=dev) for _ in range(4))
    mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
    part = torch.empty(call("triad_preln_bwd_blocks", M) * 2 * D, device=dev)
    st = stream_ptr(torch.device(dev))
    f = _event_ms(lambda: call("triad_preln_fwd", ptr(res), ptr(y), ptr(w), ptr(b), 1e-5, M, D, 0.1, 7, ptr(z), ptr(n), 0,
                               ptr(mean), ptr(rstd), st))
    g = _event_ms(lambda: call("triad_preln_bwd", ptr(dz), ptr(dn), 0, ptr(z), ptr(mean), ptr(rstd), ptr(w), M, D, 0.1, 7,
                               ptr(dres), ptr(dy), ptr(part), st))
    e = M * D
    print(f"kernels at {M} x {D}: preln_fwd {1e3 * f:.1f} us = {8 * e / f / 1e9:.2f} TB/s of 8 B/element; "
          f"preln_bwd {1e3 * g:.1f} us = {10 * e / g / 1e9:.2f} TB/s of 10 B/element")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", type=lambda s: tuple(int(v) for v in s.split(",")), default=(32, 8))
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    hub = Mdl.hubert_execution_tweaks(Mdl._hf_model("HubertModel", "facebook/hubert-large-ls960-ft", Mdl._HUBERT_LARGE))
    enc = hub.encoder.to("cuda").train()
    fused, stock = enc.forward, enc._triad_stock_forward
    assert fused.__func__ is postln._stable_encoder_forward
    default = postln.STABLE_ROUTE
    postln.STABLE_ROUTE = True      # the fused side is timed whatever the default is
    print(f"device {torch.cuda.get_device_name(0)}; HuBERT-large encoder, {len(enc.layers)} layers, {TOKENS} tokens; "
          f"STABLE_ROUTE default {default}; rounds {a.rounds} x iters {a.iters}, ms per forward + backward")
    for B in a.batches:
        x = torch.randn(B, TOKENS, enc.config.hidden_size, device="cuda").to(torch.bfloat16).requires_grad_(True)
        gy = torch.randn(B, TOKENS, enc.config.hidden_size, device="cuda")
        for _ in range(2):           # warm-up: two rounds of each at this shape, not reported
            for fwd in (fused, stock):
                _time(enc, fwd, x, gy, a.iters, 100)
        t = {"fused": [], "stock": []}
        for _ in range(a.rounds):
            t["fused"].append(_time(enc, fused, x, gy, a.iters, 100))
            t["stock"].append(_time(enc, stock, x, gy, a.iters, 100))
        enc.forward = fused
        med = {n: statistics.median(v) for n, v in t.items()}
        spread = {n: (max(v) - min(v)) / med[n] for n, v in t.items()}
        print(f"B {B} ({B * TOKENS} rows): fused {med['fused']:.2f} ms (spread {100 * spread['fused']:.1f} %), "
              f"stock {med['stock']:.2f} ms (spread {100 * spread['stock']:.1f} %), fused / stock "
              f"{med['fused'] / med['stock']:.3f}")
        print("   fused rounds:", " ".join(f"{v:.2f}" for v in t["fused"]))
        print("   stock rounds:", " ".join(f"{v:.2f}" for v in t["stock"]))
        if a.kernels:
            _kernels(B * TOKENS)


if __name__ == "__main__":
    main()
