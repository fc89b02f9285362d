"""fp64 references, derived bounds, seeded cases and plain-torch emulations for the pre-LN (stable
layer norm) kernels of csrc/postln.hip (triad_preln_fwd / _bwd). No device needed:
tests/test_preln_gpu.py applies the references and bounds to what the kernels return,
tests/test_preln_checks_cpu.py applies them to the emulations below, intact (must pass) and with one
planted error each (must fail). The keep bits, the dropped term, the wave-order row sums and the
LayerNorm bounds are those of tests/postln_ref.py (imported, not copied).

What is exact. res and y are bf16, scale = fl32(1 / fl32(1 - fl32(p))). The code forms
    yd = keep ? bf16(fl32(float(y) scale)) : 0          (postln_ref.dropped restates both roundings)
    z  = bf16(fl32(float(res) + yd))
The sum of two bf16 values is exact in fp64, so both roundings of z are restated on an exact value and
z is known bit for bit: res_out must EQUAL it (it is also what torch's bf16 add gives: the fp32 sum
rounded to bf16). Without y, z = res.

Forward, u = 2^-24. The statistics run over float(z), which holds z exactly, so the row error ez of
postln_ref is 0 and its forward bound applies with res := z, y := 0, p := 0 (h = D / 64 + 5 roundings
on the longest path of a row sum, two-pass variance, rsqrtf 2 ulp), A = mean|z|:
    mean:  dm = (h + 1) u A
    rstd:  relative rel_r = 0.5 (dm rstd)^2 + (0.5 (h + 6) + 4) u
    n f32: |w| rstd dm + |xhat w| (rel_r + 4 u) + u |ref|
    n bf16: the same + 2^-8 |ref|
Identity read from the code: the fp32 form and the bf16 form compute the same fp32 n and the bf16 form
rounds it once, so bf16(n_f32) == n_bf16 bit for bit across two calls.

Backward, mean / rstd fp32 operands (the fp64 statistics rounded to fp32). dn is one tensor (bf16 or
fp32, both exact in fp64), so postln_ref's backward bound applies with dl := dn, edl = 0, res := z:
    L = LN'(dn) = rstd (wd - c1 - xh c2): (ref_L, e_L) = postln_ref.dropaddln_bwd_ref(...)["dres"]
    g = float(dz) + L in fp32: one more rounding (none when dz or dn is NULL: the sum has one term)
        e_g = e_L + u |g|
    dres = bf16(g): e_g + 2^-8 |g|
    part / total: postln_ref's, per block of the same grid-stride loop (zero without dn)
Identity: dy == keep ? bf16(fl32(float(dres) scale)) : 0 of the kernel's own bf16 dres
(postln_ref.dy_of). None of the bounds is fitted to what a kernel returns.
"""
import torch

from tests import postln_ref as R

BF, F32, F64, U, R8 = R.BF, R.F32, R.F64, R.U, R.R8
EPS = R.EPS
FWD_DS = (256, 512, 768, 1024)
FWD_MS = (1, 3, 4, 5, 130)
FWD_PS = (0.0, 0.1, 0.5)
BWD_BIG = ((4101, 256), (4101, 1024), (8197, 256))   # past one grid-stride trip; NB = 4; a partial third trip
BWD_MODES = (("dz",), ("dn",), ("dz", "dn"))
SEED_HI = R.SEED_HI    # >= 2^31


def preln_case(M, D):
    """postln_ref.postln_case with the stream in bf16: res, y bf16; w, b fp32; dz bf16 (the gradient on
    the stream), dn bf16 and dn32 fp32 (the gradient on n in its two forms)."""
    c = R.postln_case(M, D)
    return dict(res=c["res"].to(BF), y=c["y"], w=c["w"], b=c["b"], dz=c["dhb"], dn=c["dh"].to(BF), dn32=c["dh"])


def stream(res, y, p, seed):
    """(z bf16 exact, keep bool, scale): z = bf16(fl32(res + yd)); y None: z = res."""
    if y is None:
        return res, None, 1.0
    keep = R.keep_mask(res.shape, p, seed)
    scale = R.drop_scale(p)
    return (res.double() + R.dropped(y, keep, scale)).to(F32).to(BF), keep, scale


def _zeros_like_y(z):
    return torch.zeros(z.shape, dtype=BF)


def preln_fwd_ref(res, y, w, b, eps, p, seed):
    """-> {"z": bf16 exact, "mean", "rstd", "n32", "nb": (ref, bound)}."""
    z, _, _ = stream(res, y, p, seed)
    want = R.dropaddln_fwd_ref(z.float(), _zeros_like_y(z), w, b, eps, 0.0, 0)
    assert bool(want["exact"].all())
    return {"z": z, "mean": want["mean"], "rstd": want["rstd"], "n32": want["h"], "nb": want["hb"]}


def ref_stats(z, w, b, eps):
    """The fp64 statistics of z rounded to fp32: the backward's operands."""
    want = R.dropaddln_fwd_ref(z.float(), _zeros_like_y(z), w, b, eps, 0.0, 0)
    return want["mean"][0].to(F32), want["rstd"][0].to(F32)


def preln_bwd_ref(dz, dn, z, mean, rstd, w):
    """dz bf16 or None, dn bf16 / fp32 or None (not both None) -> {"dres": (ref g, bound of the bf16
    dres), "part": (ref [blocks][2][D], bound), "total": (ref [2][D], bound)}."""
    M, D = z.shape
    G = R.bwd_blocks(M)
    if dn is None:
        L, eL = torch.zeros(M, D, dtype=F64), torch.zeros(M, D, dtype=F64)
        part = (torch.zeros(G, 2, D, dtype=F64), torch.zeros(G, 2, D, dtype=F64))
        total = (torch.zeros(2, D, dtype=F64), torch.zeros(2, D, dtype=F64))
    else:
        f32 = dn.dtype == F32
        want = R.dropaddln_bwd_ref(dn if f32 else None, None if f32 else dn, z.float(), _zeros_like_y(z), mean, rstd,
                                   w, 0.0, 0)
        (L, eL), part, total = want["dres"], want["part"], want["total"]
    g = L if dz is None else dz.double() + L
    eg = eL + (U * g.abs() if (dz is not None and dn is not None) else 0.0)
    return {"dres": (g, eg + R8 * g.abs()), "part": part, "total": total}


def emul_preln_fwd(res, y, w, b, eps, p, seed, out_f32, z_unrounded=False, yd_unrounded=False):
    """(res_out bf16, n, mean, rstd) in the kernel's operation order. Planted errors: z_unrounded (the
    statistics and n from the fp32 sum, not from its bf16 rounding), yd_unrounded (the dropout output
    not rounded to bf16 before the add)."""
    if y is None:
        s = res.float()
    else:
        keep = R.keep_mask(res.shape, p, seed)
        yd = y.float() * torch.tensor(R.drop_scale(p), dtype=F32)
        if not yd_unrounded:
            yd = yd.to(BF).float()
        s = res.float() + torch.where(keep, yd, torch.zeros_like(yd))
    zb = s.to(BF)
    v = s if z_unrounded else zb.float()
    n32, nb, mean, rstd = R.emul_dropaddln_fwd(v, _zeros_like_y(v), w, b, eps, 0.0, 0)
    return zb, (n32 if out_f32 else nb), mean, rstd


def emul_preln_bwd(dz, dn, z, mean, rstd, w, p, seed, has_y=True, ignore_dz=False, ignore_dn=False,
                   dy_unrounded=False, no_c2=False):
    """(dres bf16, dy bf16 or None, part [blocks][2][D] fp32) in the kernel's operation order; one planted
    error per keyword."""
    M, D = z.shape
    if dn is None or ignore_dn:
        L, part = torch.zeros(M, D), torch.zeros(R.bwd_blocks(M), 2, D)
    else:
        f32 = dn.dtype == F32
        L, _, part = R.emul_dropaddln_bwd(dn if f32 else None, None if f32 else dn, z.float(), _zeros_like_y(z), mean,
                                          rstd, w, 0.0, 0, no_c2=no_c2)
    g = L if (dz is None or ignore_dz) else dz.float() + L
    dres = g.to(BF)
    if not has_y:
        return dres, None, part
    keep = R.keep_mask(z.shape, p, seed)
    t = ((g if dy_unrounded else dres.float()) * torch.tensor(R.drop_scale(p), dtype=F32)).to(BF)
    return dres, torch.where(keep, t, torch.zeros_like(t)), part


def pick(c, mode):
    """(dz, dn) of a case for a backward mode: a tuple out of "dz", "dn", "dn32"."""
    return (c["dz"] if "dz" in mode else None), (c["dn32"] if "dn32" in mode else c["dn"] if "dn" in mode else None)


# ---- LayerDrop -------------------------------------------------------------------------------------------

def stock_layerdrop(n_layers, layerdrop, training=True):
    """The indices the stock loop of HubertEncoderStableLayerNorm.forward executes: per layer, in layer
    order, `dropout_probability = torch.rand([])` and skip iff training and it is < layerdrop."""
    kept = []
    for i in range(n_layers):
        dropout_probability = torch.rand([])
        skip_the_layer = training and dropout_probability < layerdrop
        if not skip_the_layer:
            kept.append(i)
    return kept


def layerdrop_seed(n_layers=6, layerdrop=0.5):
    """The first torch.manual_seed for which the stock loop skips the last layer and an interior one and
    still runs at least two layers, one of them after a skipped one."""
    for s in range(1000):
        torch.manual_seed(s)
        kept = stock_layerdrop(n_layers, layerdrop)
        interior = [i for i in range(1, n_layers - 1) if i not in kept]
        if n_layers - 1 not in kept and interior and len(kept) >= 2 and max(kept) > min(interior):
            return s, kept
    raise AssertionError("no such seed below 1000")
