"""Forward + backward time of the DistilBERT TextEmbedder on padded (ragged) caption batches, under bf16
autocast in training mode: B = 256 captions of Nt = 32 tokens (the c3 text shape) and of Nt = 128 (the
tokenizer's max_length), lengths drawn as tests/test_configs_gpu.py::_inputs draws them (uniform in
[Nt / 2, Nt], sample 0 full), the pre-tokenised batch on the host as a data loader hands it over.

With the key-padding mask in the attention kernels such a batch runs the fused transformer
(postln._distilbert_transformer_forward, triad_attn_fwd_keymask); before it, the stock transformers loop.
The script prints which attention entry points one step launched, so a log shows the path it timed. To
compare two commits, run it from a checkout of each, alternating process by process on one box:

    python tools/text_ragged_time.py [--rounds 7] [--iters 10] [--shapes 256x32,256x128]
"""
import argparse
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from triad_amd import attention as A  # noqa: E402
from triad_amd.model import TextEmbedder  # noqa: E402


def _batch(B, ntok):
    ids = torch.randint(1000, 30522, (B, ntok), generator=torch.Generator().manual_seed(5))
    lens = torch.randint(ntok // 2, ntok + 1, (B,), generator=torch.Generator().manual_seed(6))
    lens[0] = ntok
    return {"input_ids": ids, "attention_mask": (torch.arange(ntok)[None] < lens[:, None]).long()}


def _step(emb, batch):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        feats, _ = emb(batch)
    feats.float().square().mean().backward()
    emb.zero_grad(set_to_none=True)


def _time(emb, batch, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        _step(emb, batch)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _launched(emb, batch):
    seen, real = {}, A.call

    def counting(name, *a, **k):
        seen[name] = seen.get(name, 0) + 1
        return real(name, *a, **k)
    A.call = counting
    try:
        _step(emb, batch)
    finally:
        A.call = real
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default="256x32,256x128")
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    torch.manual_seed(0)
    emb = TextEmbedder(embedding_dim=512, model_name="distilbert/distilbert-base-uncased").to("cuda").train()
    print(f"device {torch.cuda.get_device_name()}; rounds {args.rounds} x iters {args.iters}, ms per forward + backward")
    for shape in args.shapes.split(","):
        B, ntok = (int(x) for x in shape.split("x"))
        batch = _batch(B, ntok)
        for _ in range(3):
            _step(emb, batch)
        seen = _launched(emb, batch)
        torch.cuda.synchronize()
        ms = [_time(emb, batch, args.iters) for _ in range(args.rounds)]
        med = statistics.median(ms)
        print(f"B {B} Nt {ntok} padded: {med:.3f} ms (spread {100 * (max(ms) - min(ms)) / med:.1f} %); attention entry "
              f"points per step: {seen if seen else 'none (stock transformers loop)'}")
        print("   rounds:", " ".join(f"{x:.3f}" for x in ms))


if __name__ == "__main__":
    main()
