"""fp64 references, derived per-element bounds and fp32 emulations for the ViT row kernels of
csrc/lora.hip (triad_rows_nt, triad_lora_update, triad_lora_tn) and csrc/resid_ln.hip
(triad_addln_fwd, triad_addln_bwd). No device needed: tests/test_vit_rows_conformance_gpu.py
applies the references and bounds to what the kernels return, tests/test_vit_rows_checks_cpu.py
applies them to the emulations below, intact (must pass) and with one planted error (must fail).

Every reference is computed in fp64 from the operands the kernel reads (bf16 / fp32 values, exact
in fp64). Bounds are first-order, u = 2^-24, and follow the rounding steps of the code:

* bf16 x bf16 products are exact in fp32. An fp32 sum of n of them in any order errs by at most
  (n - 1) u sum|terms|; a sum whose order is known errs by at most h u sum|terms|, h the number of
  roundings on the longest path to the result. A factor 2 covers an MFMA accumulator that does not
  round like IEEE at every step. One store to bf16 adds 2^-8 |ref|.
* rows_nt  (K-deep MFMA sum, bf16 store): 2 (K + 2) u (|X| . |W|) + 2^-8 |ref|.
* lora_update (fp32 y, 8 fmaf, bf16 store): 2 (8 + 2) u (|y| + |T| . |Bs|) + 2^-8 |ref|.
* lora_tn out (fp32): 2 (n + 2) u |alpha| (|Y|^T . |T|), n = min(M + G, 32 per + ceil(G / 16) + 18):
  M + G is the any-order count over all rows and the G = triad_lora_tn_blocks(M) slabs; the second
  form is the depth the code has -- one block's MFMA chain holds 32 per rows (per = tiles per
  block), slab_sum_kernel adds at most ceil(G / 16) slabs per lane, then (a0 + a1) + (a2 + a3) and a
  16-term chain. At M = 32 805 the any-order count would let a whole dropped tile through (it is
  0.04 of that bound); the depth form is 160 x tighter there. + 2: alpha and one spare.
* lora_tn dt (bf16): 2 (O + 8 + 2) u (|Y| . |Wt|) + 2^-8 |ref|  (O-deep sum over 8 waves' partials).
* addln forward, per row of D = 256 NB values v = xn, A = mean|v|, h = D / 64 + 5 (a lane adds its
  4 NB values in turn, wave_sum adds 6 butterfly levels):
      mean:  |dm| <= (h + 1) u A                              (+ 1: the division)
      rstd:  relative 0.5 (dm rstd)^2 + (0.5 (h + 6) + 4) u
             (sum (v - m^)^2 = sum (v - m)^2 + D dm^2 exactly; d = v - m^ and d * d round, h + 1
             fmaf / butterfly steps, the division and the eps add: (h + 6) u on var + eps, halved
             by the square root; 4 u = two ulp for rsqrtf)
      ln:    |w| rstd dm + |xhat w| (rel_rstd + 4 u) + u |ref|   [+ 2^-8 |ref| for bf16]
  The first term is the cancellation term: the error of v - mean is u-sized against |v| and |mean|
  (A), not against the difference, so it scales with u A rstd |w| and not with |ref|.
* addln backward, from the forward's own fp32 mean / rstd (exact inputs), wd = w dln,
  W1 = mean|wd|, W2 = mean|wd xhat|, T = |wd| + |c1| + |xhat c2|:
      dx: rstd (u |wd| + (h + 2) u W1 + |xhat| (h + 5) u W2 + 3 u |xhat c2| + 3 u T) + u |ref|
  (wd rounds once; c1 = sum / D over h steps; c2 the same over products of a twice-rounded xhat;
  two subtractions and the rstd multiply on T; the add to dres).
"""
import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
R8 = 2.0 ** -8
TN_WIDTHS = (1, 2, 3, 4, 6, 8, 9, 12)   # O / 256 that triad_lora_tn has an instance for


def f32(v):
    """The fp32 value a C float argument takes, as a Python float."""
    return float(torch.tensor(v, dtype=F32))


def ratio(got, ref, bound):
    """Largest err / bound over the elements (NaN if anything is not finite)."""
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    return float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())


def passes(got, ref, bound):
    r = ratio(got, ref, bound)
    return r == r and r <= 1.0


# ---- csrc/lora.hip ------------------------------------------------------------------------------

def rows_nt_ref(X, W):
    """X [M][K], W [J][K] bf16 -> (ref [M][J], bound)."""
    K = X.shape[1]
    ref = X.double() @ W.double().t()
    absprod = X.double().abs() @ W.double().abs().t()
    return ref, 2.0 * (K + 2) * U * absprod + R8 * ref.abs()


def lora_update_ref(Y, T, Bs):
    """Y [M][O], T [M][8], Bs [O][8] bf16 -> (ref of Y + T Bs^T, bound)."""
    ref = Y.double() + T.double() @ Bs.double().t()
    mag = Y.double().abs() + T.double().abs() @ Bs.double().abs().t()
    return ref, 2.0 * (8 + 2) * U * mag + R8 * ref.abs()


def tn_blocks(M):
    return min((M + 31) // 32, 512)


def tn_per(M):
    tiles = (M + 31) // 32
    return -(-tiles // tn_blocks(M))


def lora_tn_out_ref(Y, T, alpha):
    """Y [M][O], T [M][8] bf16, alpha the fp32 value -> (ref [O][8], bound)."""
    M = Y.shape[0]
    G, per = tn_blocks(M), tn_per(M)
    n = min(M + G, 32 * per + -(-G // 16) + 18)
    ref = alpha * (Y.double().t() @ T.double())
    absprod = abs(alpha) * (Y.double().abs().t() @ T.double().abs())
    return ref, 2.0 * (n + 2) * U * absprod


def lora_tn_dt_ref(Y, Wt):
    """Y [M][O], Wt [16][O] bf16 (rows 8..15 zero) -> (ref [M][8], bound)."""
    O = Y.shape[1]
    W8 = Wt[:8].double()
    ref = Y.double() @ W8.t()
    absprod = Y.double().abs() @ W8.abs().t()
    return ref, 2.0 * (O + 8 + 2) * U * absprod + R8 * ref.abs()


def emul_rows_nt(X, W, drop_kstep=None):
    Xf = X.float().clone()
    if drop_kstep is not None:
        Xf[:, 32 * drop_kstep:32 * drop_kstep + 32] = 0
    return (Xf @ W.float().t()).to(BF)


def emul_lora_update(Y, T, Bs, swap=None):
    """fp32 y, the 8 rank terms added in turn, one bf16 store. swap = j: rank columns j, j + 1 of T
    exchanged."""
    cols = list(range(8))
    if swap is not None:
        cols[swap], cols[swap + 1] = cols[swap + 1], cols[swap]
    a = Y.float()
    Tf, Bf = T.float(), Bs.float()
    for j in range(8):
        a = a + Tf[:, cols[j]:cols[j] + 1] * Bf[:, j]
    return a.to(BF)


def emul_lora_tn(Y, T, Wt, alpha, drop_tile=None, drop_slab=None, alpha_twice=False):
    """Per block an fp32 Y^T T over its 32-row tiles, the slabs summed in fp32, alpha once; dt the
    fp32 Y Wt^T stored as bf16. alpha is a Python float holding the fp32 value."""
    M = Y.shape[0]
    G, per = tn_blocks(M), tn_per(M)
    Yf, Tf = Y.float(), T.float()
    if drop_tile is not None:
        Yf = Yf.clone()
        Yf[32 * drop_tile:32 * drop_tile + 32] = 0
    slabs = []
    for blk in range(G):
        r0, r1 = 32 * per * blk, min(M, 32 * per * (blk + 1))
        if blk == drop_slab or r0 >= r1:
            slabs.append(torch.zeros(Y.shape[1], 8))
        else:
            slabs.append(Yf[r0:r1].t() @ Tf[r0:r1])
    a = torch.tensor(alpha, dtype=F32)
    slabs += [torch.zeros_like(slabs[0])] * (-G % 16)
    out = a * torch.stack(slabs).view(-1, 16, Y.shape[1], 8).sum(0).sum(0)   # slab lane i % 16, then the 16 lanes
    if alpha_twice:
        out = a * out
    dt = None if Wt is None else (Y.float() @ Wt[:8].float().t()).to(BF)
    return out, dt


# ---- csrc/resid_ln.hip --------------------------------------------------------------------------

def _wave_row_sum(v):
    """Row sums of v [M][D] fp32 in the kernels' order: lane l adds its values (block i, columns
    256 i + 4 l .. + 3) in turn, then the 64 lanes' sums go through wave_sum's xor butterfly."""
    M, D = v.shape
    per = v.reshape(M, D // 256, 64, 4).permute(0, 2, 1, 3).reshape(M, 64, D // 64)
    s = per[:, :, 0].clone()
    for k in range(1, D // 64):
        s = s + per[:, :, k]
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, 0]


def addln_xn(x, y, g):
    """torch's unfused fp32 x + g * y.float() (what the kernel's __fmul_rn / __fadd_rn give)."""
    return x + g * y.float()


def addln_fwd_ref(xn, w, b, eps, out_bf16):
    """xn [M][D], w, b [D] fp32, eps the fp32 value -> dict of (ref, bound) for mean, rstd, ln."""
    v = xn.double()
    D = v.shape[1]
    h = D // 64 + 5
    m = v.mean(1)
    var = ((v - m[:, None]) ** 2).mean(1)
    rstd = (var + eps) ** -0.5
    dm = (h + 1) * U * v.abs().mean(1)
    rel_r = 0.5 * (dm * rstd) ** 2 + (0.5 * (h + 6) + 4) * U
    xhat = (v - m[:, None]) * rstd[:, None]
    wd = w.double()
    ref = xhat * wd + b.double()
    bound = wd.abs() * (rstd * dm)[:, None] + (xhat * wd).abs() * (rel_r[:, None] + 4 * U) + U * ref.abs()
    if out_bf16:
        bound = bound + R8 * ref.abs()
    return {"mean": (m, dm), "rstd": (rstd, rstd * rel_r), "ln": (ref, bound)}


def emul_addln_fwd(x, y, g, w, b, eps, out_bf16, one_pass=False):
    """(xn, ln, mean, rstd) in fp32 with the kernel's summation order. one_pass: the variance as
    E[v^2] - mean^2 (the planted error)."""
    xn = x if y is None else addln_xn(x, y, g)
    D = xn.shape[1]
    mean = _wave_row_sum(xn) / D
    if one_pass:
        var = _wave_row_sum(xn * xn) / D - mean * mean
    else:
        d = xn - mean[:, None]
        var = _wave_row_sum(d * d) / D
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=F32))
    ln = (xn - mean[:, None]) * rstd[:, None] * w + b
    return xn, (ln.to(BF) if out_bf16 else ln), mean, rstd


def addln_bwd_ref(dln, dres, xn, mean, rstd, w):
    """dln [M][D] (bf16 or fp32), dres [M][D] fp32 or None, xn, mean, rstd, w fp32 (mean / rstd the
    forward's outputs, taken as exact inputs) -> (ref dx, bound)."""
    D = xn.shape[1]
    h = D // 64 + 5
    r = rstd.double()[:, None]
    xh = (xn.double() - mean.double()[:, None]) * r
    wd = w.double() * dln.double()
    c1 = wd.mean(1, keepdim=True)
    c2 = (wd * xh).mean(1, keepdim=True)
    ref = r * (wd - c1 - xh * c2)
    if dres is not None:
        ref = ref + dres.double()
    W1 = wd.abs().mean(1, keepdim=True)
    W2 = (wd * xh).abs().mean(1, keepdim=True)
    T = wd.abs() + c1.abs() + (xh * c2).abs()
    bound = r * (U * wd.abs() + (h + 2) * U * W1 + xh.abs() * (h + 5) * U * W2 + 3 * U * (xh * c2).abs()
                 + 3 * U * T) + U * ref.abs()
    return ref, bound


def addln_dy(dx, g):
    """dy as the kernel forms it: bf16 of the fp32 product g * dx."""
    return (g * dx).to(BF)


def emul_addln_bwd(dln, dres, xn, mean, rstd, w, g, no_c2=False, dy_before_dres=False):
    """(dx, dy) in fp32 with the kernel's summation order; the two planted errors by keyword."""
    D = xn.shape[1]
    xh = (xn - mean[:, None]) * rstd[:, None]
    wd = w * dln.float()
    c1 = (_wave_row_sum(wd) / D)[:, None]
    c2 = (_wave_row_sum(wd * xh) / D)[:, None]
    inner = wd - c1 if no_c2 else wd - c1 - xh * c2
    lnb = rstd[:, None] * inner
    dx = lnb if dres is None else dres + lnb
    dy = addln_dy(lnb if dy_before_dres else dx, g)
    return dx, dy


# ---- vit.LoRALinear -----------------------------------------------------------------------------

def bf16_flip(v, e):
    """For fp64 values v known to within e: (bf16(v) as fp64, the distance another value within e
    of v can round away from it: 0 where v - e .. v + e rounds to one bf16 value, else the gap).
    The 2 u |v| covers the fp32 step of the cast."""
    e = e + 2 * U * v.abs()
    lo, hi = (v - e).to(F32).to(BF).double(), (v + e).to(F32).to(BF).double()
    return v.to(F32).to(BF).double(), hi - lo


def lora_linear_ref(x, W, b, A, sB, s, dy):
    """fp64 reference and per-element bounds of _LoRALinear's forward and backward for bf16-valued
    x [M][K], W [O][K], b [O], A [8][K], sB = s B [O][8] (s the LoRA scaling) and dy [M][O], with
    the two intermediates the product stores as bf16 rounded: t = bf16(x A^T), dt = bf16(dy sB).

        y  = bf16(bf16(x W^T + b) + t sB^T)        base GEMM, then triad_lora_update
        dB = s dy^T t                              triad_lora_tn with alpha = s
        dx = bf16(bf16(dy W) + dt A)
        dA = dt^T x

    The kernel's t (dt) differs from the reference's only where the fp64 value lies within the
    fp32 sum's bound of a bf16 rounding boundary: there by one bf16 gap (bf16_flip), elsewhere not
    at all. That distance, times the other operand, is added to every bound that consumes t or dt.
    The window uses the depth the code has, not the any-order count, to flag as few elements as the
    code allows: rows_nt chains K / 32 MFMAs of 32 products each (K / 32 + 32), lora_tn's dt chains
    O / 256 such MFMAs per wave and adds the 8 waves (O / 256 + 32 + 8). dA and dB stay far inside
    their bounds (no element does flip, the bound has to allow every flagged one); one row left out
    of either sum still exceeds them (test_vit_rows_checks_cpu.py).
    Returns {name: (ref, bound)} for y, dx, dA, dB."""
    xd, Wd, Ad, Bd, dyd = (t.double() for t in (x, W, A, sB, dy))
    M, K = xd.shape
    O = Wd.shape[0]
    G = tn_blocks(M)
    tn = 2.0 * (min(M + G, 32 * tn_per(M) + -(-G // 16) + 18) + 2) * U
    upd = 2.0 * (8 + 2) * U
    # forward
    t, et = bf16_flip(xd @ Ad.t(), 2.0 * (K // 32 + 32 + 2) * U * (xd.abs() @ Ad.abs().t()))
    base = xd @ Wd.t() + b.double()
    ebase = 2.0 * (K + 2) * U * (xd.abs() @ Wd.abs().t() + b.double().abs()) + R8 * base.abs()
    y = base + t @ Bd.t()
    ey = ebase + upd * (base.abs() + t.abs() @ Bd.abs().t()) + et @ Bd.abs().t() + R8 * y.abs()
    # backward
    dt, edt = bf16_flip(dyd @ Bd, 2.0 * (O // 256 + 32 + 8 + 2) * U * (dyd.abs() @ Bd.abs()))
    dB = s * (dyd.t() @ t)
    edB = abs(s) * (tn * (dyd.abs().t() @ t.abs()) + dyd.abs().t() @ et)
    dxb = dyd @ Wd
    edxb = 2.0 * (O + 2) * U * (dyd.abs() @ Wd.abs()) + R8 * dxb.abs()
    dx = dxb + dt @ Ad
    edx = edxb + upd * (dxb.abs() + dt.abs() @ Ad.abs()) + edt @ Ad.abs() + R8 * dx.abs()
    dA = dt.t() @ xd
    edA = tn * (dt.abs().t() @ xd.abs()) + edt.t() @ xd.abs()
    return {"y": (y, ey), "dx": (dx, edx), "dA": (dA, edA), "dB": (dB, edB)}


# ---- seeded operands (CPU), shared by the GPU and the CPU tests ----------------------------------

def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1000003 + int(k)
    return torch.Generator().manual_seed(seed % (2 ** 31))


def rows_nt_case(M, K, J):
    g = _gen(1, M, K, J)
    return torch.randn(M, K, generator=g).to(BF), torch.randn(J, K, generator=g).to(BF)


def lora_update_case(M, O):
    """Y [M][O], T [M][8], Bs [O][8]: every rank column of T and Bs its own values."""
    g = _gen(2, M, O)
    return (torch.randn(M, O, generator=g).to(BF), torch.randn(M, 8, generator=g).to(BF),
            (torch.randn(O, 8, generator=g) * 0.5).to(BF))


def lora_tn_case(M, O):
    """Y [M][O], T [M][8] (all 8 rank columns filled), Wt [16][O] with rows 8..15 zero."""
    g = _gen(3, M, O)
    Y = torch.randn(M, O, generator=g).to(BF)
    T = torch.randn(M, 8, generator=g).to(BF)
    Wt = torch.zeros(16, O, dtype=BF)
    Wt[:8] = torch.randn(8, O, generator=g).to(BF)
    return Y, T, Wt


SPECIAL_ROWS = {"mean100": 0, "tiny": 1, "const": 2}   # rows of an addln case with D = 768, M >= 4
CONST = 2.5   # every partial sum of 768 of them is exact in fp32


def addln_case(M, D):
    """x fp32, y bf16, g of varied sign and magnitude (1e-3 .. 2), w, b, dln (bf16 and fp32), dres.
    At D = 768 and M >= 4 rows 0..2 are: mean 100 with sigma 0.1, mean 0 with sigma 1e-3, constant."""
    g = _gen(4, M, D)
    x = torch.randn(M, D, generator=g) * 1.5 + 0.3
    y = torch.randn(M, D, generator=g)
    gam = torch.randn(D, generator=g).sign() * 10.0 ** (torch.rand(D, generator=g) * 3.3 - 3.0)
    if D == 768 and M >= 4:
        x[0] = 100.0 + 0.1 * torch.randn(D, generator=g)
        y[0] *= 0.01
        x[1] = 1e-3 * torch.randn(D, generator=g)
        x[2] = CONST
        y[1:3] = 0
    w = 1.0 + 0.5 * torch.randn(D, generator=g)
    b = 0.3 * torch.randn(D, generator=g)
    dln = torch.randn(M, D, generator=g)
    dres = torch.randn(M, D, generator=g)
    return dict(x=x, y=y.to(BF), g=gam, w=w, b=b, dln_f32=dln, dln_bf16=dln.to(BF), dres=dres)
