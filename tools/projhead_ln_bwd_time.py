"""Device time of triad_projhead_ln_bwd alone (the row-panel head's LayerNorm-backward GEMM,
csrc/rowgemm.hip) at the step's row counts, by device events around `iters` back-to-back launches after
a warm-up; operands are the forward's own buffers (triad_projhead_fwd at H = 768). One JSON line per
row count. For an A/B, run it alternately with TRIAD_LIB_VARIANT unset / set to another build of the
library (tools/build_variants.py) in one session and compare within that log only; --digest also
prints a checksum of dy1 and the partials, equal between two builds that compute the same bits."""
import argparse
import hashlib
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[65536, 8192])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--tag", default="prod")
    ap.add_argument("--digest", action="store_true")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from triad_amd._lib import call, ptr, stream_ptr
    dev, bf, H, D = "cuda", torch.bfloat16, 768, 512
    for M in a.rows:
        g = torch.Generator(device=dev).manual_seed(M)
        h = torch.randn(M, H, device=dev, generator=g).to(bf)
        w1 = (torch.randn(D, H, device=dev, generator=g) / H ** 0.5).to(bf)
        w2 = (torch.randn(D, D, device=dev, generator=g) / D ** 0.5).to(bf)
        b = (torch.randn(D, device=dev, generator=g) * 0.1).to(bf)
        gam, bet = torch.rand(D, device=dev, generator=g) + 0.5, torch.randn(D, device=dev, generator=g) * 0.1
        dy = (torch.randn(M, D, device=dev, generator=g) * 0.01).to(bf)
        P = call("triad_rowpanel_count", M)
        Mp = P * 128
        st = stream_ptr()
        w1p, w2p, w2b = (torch.empty(n, dtype=bf, device=dev) for n in (H * D, D * D, D * D))
        call("triad_wpack2", ptr(w1), H, ptr(w1p), ptr(w2), D, ptr(w2p), st)
        call("triad_bfrag_pack16", ptr(w2), D // 32, 1, ptr(w2b), st)
        y1, ln, y, dy1 = (torch.empty(Mp, D, dtype=bf, device=dev) for _ in range(4))
        mean, rstd = torch.empty(Mp, device=dev), torch.empty(Mp, device=dev)
        part = torch.empty(P, 3, D, device=dev)
        call("triad_projhead_fwd", ptr(h), M, H, H, M, 0, ptr(w1p), ptr(b), ptr(gam), ptr(bet), 1e-5, ptr(w2p), ptr(b),
             ptr(y1), ptr(ln), ptr(mean), ptr(rstd), ptr(y), st)

        def run():
            call("triad_projhead_ln_bwd", ptr(dy), M, ptr(w2b), ptr(y1), ptr(mean), ptr(rstd), ptr(gam), ptr(dy1),
                 ptr(part), st)
        for _ in range(20):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.iters
        out = {"tag": a.tag, "rows": M, "iters": a.iters, "ln_bwd_us": round(us, 2),
               "TFLOPs": round(2.0 * M * D * D / us / 1e6, 1)}
        if a.digest:
            hsh = hashlib.sha256()
            for t in (dy1, part):
                hsh.update(t.cpu().view(torch.uint8).numpy().tobytes())
            out["digest"] = hsh.hexdigest()[:16]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
