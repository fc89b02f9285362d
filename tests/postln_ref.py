"""Host-side definition of the dropout keep bits, fp64 references, derived per-element bounds,
seeded cases and fp32 / bf16 emulations for the post-LN kernels of csrc/postln.hip
(triad_dropaddln_fwd / _bwd, triad_geludrop_fwd / _bwd, triad_gelu_table, triad_dropout_keep).
No device needed: tests/test_postln_conformance_gpu.py applies the references and bounds to what
the kernels return, tests/test_postln_checks_cpu.py applies them to the emulations below, intact
(must pass) and with one planted error each (must fail).

Keep bits (csrc/common.h hash32 / keep_pair / triad_drop_thr, restated in numpy uint32 arithmetic;
the device is compared with this bit for bit, and post-LN, short and long attention dropout all
prove their bits equal to triad_dropout_keep, so this is the definition they rest on):
    lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
    pair q = e >> 1 (64 bit): h = lowbias32(lo32(q) * 0x9E3779B9 + seed + lowbias32(hi32(q) ^ 0x85ebca6b))
    element 2q keeps iff (h & 0xffff) >= thr, element 2q + 1 iff (h >> 16) >= thr
    thr = (unsigned)(p * 65536.f + 0.5f) in fp32 (p * 65536 is exact, the add rounds once)

Dropped term. scale = fl32(1 / fl32(1 - fl32(p))) is an operand. The code forms
(float)(bf16)(y * scale): the exact bf16 x fp32 product (exact in fp64) rounded to fp32, then to
bf16. Both roundings are restated (a single rounding to bf16 differs where the fp32 rounding lands
on a bf16 tie, about one element in 2^16), so yd is exact and z = res + yd is exact in fp64.

Every reference is fp64 of the operands the kernel reads. Bounds are first-order, u = 2^-24, follow
the rounding steps of the code, and none is fitted to what a kernel returns. They start from the
addln derivation of tests/vit_rows_ref.py: a lane adds its D / 64 values in turn, wave_sum adds 6
butterfly levels, h = D / 64 + 5 roundings on the longest path; two-pass variance; rsqrtf 2 ulp.

Forward. The kernel's v is fl32(z), not z: ez = u |z| per element, 0 on a row where every z is an
fp32 value (dropaddln_fwd_ref checks that and returns the row mask; the mean-100 row of the cases is
built to satisfy it: res in [64, 128) lies on the 2^-17 grid, y = k / 16, so res + yd is exact).
With A = mean|z|, Ez = mean ez:
    mean:  dm = (h + 1) u A + Ez
    rstd:  relative 0.5 (dm rstd)^2 + (0.5 (h + 6) + 4) u + 0.5 rstd^2 (2 mean(|z - m| ez) + mean ez^2)
           (the last term: var of the rounded values against var of z)
    h:     |w| rstd (dm + ez) + |xhat w| (rel_rstd + 4 u) + u |ref|       [+ 2^-8 |ref| for hb]
A constant row c with exact partial sums has mean == c, every d == 0, so h == b bit for bit and
rstd = rsqrtf(eps) within (0.5 * 2 + 4) u of 1 / sqrt(eps).

Backward, mean / rstd fp32 operands (optionally known only to dm / rel_r: the chained test, where
they are the forward kernel's own and the reference keeps the fp64 statistics). dl = dh + fl32(dhb)
rounds once when both are given: edl = u |dl|, else 0. wd = w dl, xh = (z - mean) rstd:
    e_xh = rstd (ez + dm) + (2 u + rel_r) |xh|        (subtraction and product round)
    e_wd = |w| edl + u |wd|
    c1:    e_c1 = mean e_wd + (h + 1) u mean|wd|
    c2:    e_c2 = mean (e_wd |xh| + |wd| e_xh) + (h + 1) u mean|wd xh|
    dres:  rstd (e_wd + e_c1 + e_xh |c2| + |xh| e_c2 + u |xh c2| + 3 u T) + (u + rel_r) |ref|,
           T = |wd| + |c1| + |xh c2|   (the cancellation is among these three)
    part dgamma[blk]: sum_rows (edl |xh| + |dl| e_xh) + (trips + 3) u sum_rows |dl xh|
    part dbeta[blk]:  sum_rows edl + (trips + 3) u sum_rows |dl|
           (a wave's accumulator takes one fma / add per trip of the grid-stride loop, trips =
           ceil(row groups / blocks); the LDS reduction adds the 4 waves: 3 roundings)
    totals: the fp64 sum of the partials against the fp64 sum of their references, bounds summed.
Rows go to blocks as the code assigns them: row r belongs to block (r / 4) % blocks, wave r % 4.

Bit-identities read from the code: hb == bf16(h) of the kernel's own h; dy == bf16(bf16(dres) keep
scale) of its own dres; a constant row gives h == b; repeats are bit-identical (no atomics);
table == NULL and the table give identical bits; geludrop_fwd at p equals bf16(g keep scale) of the
p = 0 output g of the same kernel (the GELU value is rounded to bf16 before the dropout scaling).

GELU. fp64 reference 0.5 x erfc(-x / sqrt 2) and aten's slope cdf + x pdf. The bound is absolute:
1 + erf(t) cancels for negative t, so erff's error is relative to erf ~ -1, not to the result.
ASSUMED (HIP's published maximum errors as recalled, not verifiable in this repository, each
doubled; the same assumption as tests/frontend_ref.py; never tuned to a kernel's output): erff 4
ulp, expf 1 ulp of their results.
    E_erf       = 2 ERFF_ULP 2 u |erf t| + 2 u |t| erf'(t),  t = x / sqrt 2  (the argument's rounding)
    value  f32: gv_err = 0.5 |x| (E_erf + u |1 + erf t|) + 2 u |gelu|
    g = bf16(value): gv_err + 2^-8 |gelu| + TINY       (TINY = 2^-133, one bf16 subnormal step)
    v = bf16(g scale): scale (g's bound) + u |ref| + 2^-8 |ref| + TINY
    slope  f32: gs_err = 0.5 (E_erf + u |1 + erf t|) + |x pdf| ((2 2 EXPF_ULP + 3 |a|) u + 3 u) + 2 u |slope|,
                a = x^2 / 2   (2 |a| u: the two products forming a; |a| u: expf's argument scaling)
    du = bf16(dg slope), dg = bf16(dv scale) exact: |dg| gs_err + u |ref| + 2^-8 |ref| + TINY
"""
import math

import numpy as np
import torch

from tests.vit_rows_ref import BF, F32, F64, R8, U, _gen, _wave_row_sum, f32, passes, ratio  # noqa: F401

ERFF_ULP = 4.0    # ASSUMED
EXPF_ULP = 1.0    # ASSUMED
TINY = 2.0 ** -133
SQRT1_2 = math.sqrt(0.5)
INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)
BWD_MAX_BLOCKS = 1024
P_LIST = (0.0, 2.0 ** -18, 0.1, 0.5, 1.0 - 2.0 ** -16, 1.0 - 2.0 ** -24)   # thr 0, 0, 6554, 32768, 65535, 65536


# ---- keep bits --------------------------------------------------------------------------------------

def hash32(x):
    """lowbias32 on a numpy uint32 array (wrap-around arithmetic)."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def drop_thr(p):
    """(unsigned)(p * 65536.f + 0.5f), every step in fp32."""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def drop_scale(p):
    """fl32(1 / fl32(1 - fl32(p))) as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def pair_hash(q, seed):
    """The 32-bit hash of pairs q (numpy uint64): its low half belongs to element 2q, its high half
    to element 2q + 1."""
    q = np.asarray(q, dtype=np.uint64)
    lo = (q & np.uint64(0xffffffff)).astype(np.uint32)
    hi = (q >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = lo * np.uint32(0x9E3779B9) + np.uint32(seed & 0xffffffff) + hash32(hi ^ np.uint32(0x85ebca6b))
    return hash32(x)


def keep_fields(n, seed, start=0):
    """The 16-bit uniform of elements start .. start + n - 1 (numpy uint32)."""
    e = np.arange(start, start + n, dtype=np.uint64)
    h = pair_hash(e >> np.uint64(1), seed)
    return np.where((e & np.uint64(1)).astype(bool), h >> np.uint32(16), h & np.uint32(0xffff))


def keep_bits(n, p, seed, start=0, swap_pair=False, strict=False):
    """Keep bits (numpy bool) of n elements. Planted errors: swap_pair (element 2q takes the high
    half), strict (> thr instead of >= thr)."""
    f = keep_fields(n, seed, start)
    if swap_pair:
        assert start % 2 == 0 and n % 2 == 0
        f = f.reshape(-1, 2)[:, ::-1].reshape(-1)
    thr = drop_thr(p)
    return f > thr if strict else f >= thr


def keep_mask(shape, p, seed, **kw):
    n = int(np.prod(shape))
    return torch.from_numpy(keep_bits(n, p, seed, **kw)).view(shape)


# ---- dropaddln --------------------------------------------------------------------------------------

def dropped(y, keep, scale):
    """yd = keep ? bf16(fl32(y * scale)) : 0 as fp64 (y bf16, scale the fp32 value): both roundings
    of the code, each applied to an exact value."""
    yd = (y.double() * scale).to(F32).to(BF).double()
    return torch.where(keep, yd, torch.zeros_like(yd))


def bwd_blocks(M):
    return (M + 3) // 4 if M < 4 * BWD_MAX_BLOCKS else BWD_MAX_BLOCKS


def bwd_trips(M):
    return -(-((M + 3) // 4) // bwd_blocks(M))


def row_block(M):
    """Block of every row, as dropaddln_bwd_kernel's grid-stride loop assigns them."""
    return (torch.arange(M) // 4) % bwd_blocks(M)


def dropaddln_z(res, y, p, seed):
    """(z fp64 exact, keep bool, scale) of a case."""
    keep = keep_mask(res.shape, p, seed)
    scale = drop_scale(p)
    return res.double() + dropped(y, keep, scale), keep, scale


def dropaddln_fwd_ref(res, y, w, b, eps, p, seed):
    """res fp32 [M][D], y bf16, w, b fp32 [D], eps the fp32 value -> {"mean", "rstd", "h", "hb":
    (ref, bound), "exact": [M] bool (every z of the row is an fp32 value), "dm", "rel_r"}."""
    z, _, _ = dropaddln_z(res, y, p, seed)
    D = z.shape[1]
    h = D // 64 + 5
    exact = (z.to(F32).double() == z).all(1)
    ez = torch.where(exact[:, None], torch.zeros_like(z), U * z.abs())
    m = z.mean(1)
    c = z - m[:, None]
    var = (c * c).mean(1)
    rstd = (var + eps) ** -0.5
    dm = (h + 1) * U * z.abs().mean(1) + ez.mean(1)
    rel_r = (0.5 * (dm * rstd) ** 2 + (0.5 * (h + 6) + 4) * U
             + 0.5 * rstd ** 2 * (2 * (c.abs() * ez).mean(1) + (ez * ez).mean(1)))
    xhat = c * rstd[:, None]
    wd = w.double()
    ref = xhat * wd + b.double()
    bound = wd.abs() * rstd[:, None] * (dm[:, None] + ez) + (xhat * wd).abs() * (rel_r[:, None] + 4 * U) + U * ref.abs()
    return {"mean": (m, dm), "rstd": (rstd, rstd * rel_r), "h": (ref, bound), "hb": (ref, bound + R8 * ref.abs()),
            "exact": exact, "dm": dm, "rel_r": rel_r}


def dy_of(dres, keep, scale):
    """dy as the kernel forms it from its own fp32 dres: bf16(bf16(dres) * scale) where kept."""
    t = (dres.to(BF).float() * torch.tensor(scale, dtype=F32)).to(BF)
    return torch.where(keep, t, torch.zeros_like(t))


def dropaddln_bwd_ref(dh, dhb, res, y, mean, rstd, w, p, seed, dm=None, rel_r=None):
    """dh fp32 / dhb bf16 [M][D] (either None), mean, rstd [M] the statistics the reference uses
    (fp32 operands, or fp64 with the kernel's known only to dm / rel_r) -> {"dres": (ref, bound),
    "part": (ref [blocks][2][D], bound), "total": (ref [2][D], bound)}."""
    z, _, _ = dropaddln_z(res, y, p, seed)
    M, D = z.shape
    h = D // 64 + 5
    exact = (z.to(F32).double() == z).all(1)
    ez = torch.where(exact[:, None], torch.zeros_like(z), U * z.abs())
    dmv = torch.zeros(M, 1, dtype=F64) if dm is None else dm.double()[:, None]
    rr = torch.zeros(M, 1, dtype=F64) if rel_r is None else rel_r.double()[:, None]
    zero = torch.zeros_like(z)
    dl = (zero if dh is None else dh.double()) + (zero if dhb is None else dhb.double())
    edl = U * dl.abs() if (dh is not None and dhb is not None) else zero
    r = rstd.double()[:, None]
    xh = (z - mean.double()[:, None]) * r
    e_xh = r * (ez + dmv) + (2 * U + rr) * xh.abs()
    wv = w.double()
    wd = wv * dl
    e_wd = wv.abs() * edl + U * wd.abs()
    c1 = wd.mean(1, keepdim=True)
    c2 = (wd * xh).mean(1, keepdim=True)
    e_c1 = e_wd.mean(1, keepdim=True) + (h + 1) * U * wd.abs().mean(1, keepdim=True)
    e_c2 = (e_wd * xh.abs() + wd.abs() * e_xh).mean(1, keepdim=True) + (h + 1) * U * (wd * xh).abs().mean(1, keepdim=True)
    ref = r * (wd - c1 - xh * c2)
    T = wd.abs() + c1.abs() + (xh * c2).abs()
    bound = r * (e_wd + e_c1 + e_xh * c2.abs() + xh.abs() * e_c2 + U * (xh * c2).abs() + 3 * U * T) + (U + rr) * ref.abs()
    G, trips = bwd_blocks(M), bwd_trips(M)
    blk = row_block(M)

    def per_block(v):
        return torch.zeros(G, D, dtype=F64).index_add_(0, blk, v)
    part = torch.stack([per_block(dl * xh), per_block(dl)], 1)
    pb = torch.stack([per_block(edl * xh.abs() + dl.abs() * e_xh) + (trips + 3) * U * per_block((dl * xh).abs()),
                      per_block(edl) + (trips + 3) * U * per_block(dl.abs())], 1)
    return {"dres": (ref, bound), "part": (part, pb), "total": (part.sum(0), pb.sum(0))}


def sum_slabs_depth(S):
    """Roundings on the longest path of triad_sum_slabs over S slabs (tests/frontend_ref.py): S < 16
    four chains of ceil(S / 4) and two adds, else ceil(S / 64) + 2 + 16."""
    return -(-S // 4) + 2 if S < 16 else -(-S // 64) + 2 + 16


def emul_dropaddln_fwd(res, y, w, b, eps, p, seed, swap_pair=False, strict=False, yd_unrounded=False,
                       scale_double=False, one_pass=False):
    """(h, hb, mean, rstd) in fp32 / bf16 in the kernel's operation order; one planted error per
    keyword."""
    keep = keep_mask(res.shape, p, seed, swap_pair=swap_pair, strict=strict)
    scale = torch.tensor(1.0 / (1.0 - p) if scale_double else drop_scale(p), dtype=F32)
    yd = y.float() * scale
    if not yd_unrounded:
        yd = yd.to(BF).float()
    z = res + torch.where(keep, yd, torch.zeros_like(yd))
    D = z.shape[1]
    mean = _wave_row_sum(z) / D
    if one_pass:
        var = _wave_row_sum(z * z) / D - mean * mean
    else:
        d = z - mean[:, None]
        var = _wave_row_sum(d * d) / D
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=F32))
    h = (z - mean[:, None]) * rstd[:, None] * w + b
    return h, h.to(BF), mean, rstd


def emul_dropaddln_bwd(dh, dhb, res, y, mean, rstd, w, p, seed, no_c2=False, ignore_dh=False, ignore_dhb=False,
                       dy_unrounded=False, drop_later_trips=False, gw_unnormalised=False):
    """(dres fp32, dy bf16, part [blocks][2][D] fp32) in the kernel's operation order: a wave's
    accumulators take its rows trip by trip, the block adds its 4 waves in turn."""
    M, D = res.shape
    keep = keep_mask(res.shape, p, seed)
    scale = torch.tensor(drop_scale(p), dtype=F32)
    yd = (y.float() * scale).to(BF).float()
    z = res + torch.where(keep, yd, torch.zeros_like(yd))
    d = torch.zeros_like(res)
    if dh is not None and not ignore_dh:
        d = d + dh
    if dhb is not None and not ignore_dhb:
        d = d + dhb.float()
    rs = rstd[:, None]
    xh = (z - mean[:, None]) * rs
    wd = w * d
    c1 = (_wave_row_sum(wd) / D)[:, None]
    c2 = (_wave_row_sum(wd * xh) / D)[:, None]
    dz = rs * (wd - c1) if no_c2 else rs * (wd - c1 - xh * c2)
    t = (dz if dy_unrounded else dz.to(BF).float()) * scale
    dy = torch.where(keep, t.to(BF), torch.zeros(M, D, dtype=BF))
    G, trips = bwd_blocks(M), bwd_trips(M)
    pad = trips * G * 4 - M
    gterm = d * ((z - mean[:, None]) if gw_unnormalised else xh)

    def block_sum(v):
        v = torch.cat([v, torch.zeros(pad, D)]).view(trips, G, 4, D)
        acc = torch.zeros(G, 4, D)
        for k in range(1 if drop_later_trips else trips):
            acc = acc + v[k]
        return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    return dz, dy, torch.stack([block_sum(gterm), block_sum(d)], 1)


# ---- GELU -------------------------------------------------------------------------------------------

GL_E0, GL_NE = 127 - 40, 46
GL_N = GL_NE * 256
GL_BYTES = GL_N * 6


def gl_index(bits):
    """Host restatement of the table index of bf16 patterns (numpy int64 array): -1 = formula."""
    bits = np.asarray(bits, dtype=np.int64)
    idx = ((bits >> 7) & 255) - GL_E0
    return np.where((idx >= 0) & (idx < GL_NE), (idx << 8) | ((bits >> 8) & 128) | (bits & 127), -1)


def gl_pattern(i):
    """The bf16 pattern entry i of the table holds (the inverse of gl_index)."""
    i = np.asarray(i, dtype=np.int64)
    return (((i >> 7) & 1) << 15) | ((GL_E0 + (i >> 8)) << 7) | (i & 127)


def all_patterns():
    """Every bf16 pattern at an even and at an odd position (131 072 elements), as
    tests/test_postln_gpu.py lays them out."""
    u = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF).repeat(2)
    return torch.cat([u[1:], u[:1]])


def gelu64(x):
    return 0.5 * x * torch.special.erfc(-x * SQRT1_2)


def gelu_slope64(x):
    return 0.5 * torch.special.erfc(-x * SQRT1_2) + x * INV_SQRT_2PI * torch.exp(-0.5 * x * x)


def _erf_err(x):
    t = x * SQRT1_2
    return 2 * ERFF_ULP * 2 * U * torch.erf(t).abs() + 2 * U * t.abs() * (2 / math.sqrt(math.pi)) * torch.exp(-t * t)


def gelu_val_err(x):
    return 0.5 * x.abs() * (_erf_err(x) + U * torch.special.erfc(-x * SQRT1_2)) + 2 * U * gelu64(x).abs()


def gelu_slope_err(x):
    a = 0.5 * x * x
    xpdf = (x * INV_SQRT_2PI * torch.exp(-a)).abs()
    return (0.5 * (_erf_err(x) + U * torch.special.erfc(-x * SQRT1_2)) + xpdf * ((2 * 2 * EXPF_ULP + 3 * a) * U + 3 * U)
            + 2 * U * gelu_slope64(x).abs())


def gelu_table_ref(x):
    """x bf16 -> ((value ref, bound of the bf16 entry), (slope ref, bound of the fp32 entry))."""
    xd = x.double()
    g, s = gelu64(xd), gelu_slope64(xd)
    return (g, gelu_val_err(xd) + R8 * g.abs() + TINY), (s, gelu_slope_err(xd))


BF16_MAX = float(torch.finfo(BF).max)


def in_range(ref, bound):
    """Where a bf16 result must be finite: |ref| + bound below the largest bf16. (x scale of the 47
    largest finite patterns at p = 0.1 overflows to inf, in the code as in fp64.)"""
    return ref.abs() + bound < BF16_MAX


def geludrop_fwd_ref(u, keep, scale):
    """u bf16 (finite), keep bool, scale the fp32 value -> (ref, bound)."""
    xd = u.double()
    g = gelu64(xd)
    ref = torch.where(keep, g * scale, torch.zeros_like(g))
    eg = gelu_val_err(xd) + R8 * g.abs() + TINY
    if scale == 1.0:
        return ref, torch.where(keep, eg, torch.zeros_like(eg))
    return ref, torch.where(keep, scale * eg + (U + R8) * ref.abs() + TINY, torch.zeros_like(eg))


def geludrop_bwd_ref(u, dv, keep, scale):
    """u, dv bf16 (u finite) -> (ref, bound) of du = bf16(dg slope), dg = bf16(dv scale) where kept."""
    xd = u.double()
    dg = (dv.double() * scale).to(F32).to(BF).double()
    dg = torch.where(keep, dg, torch.zeros_like(dg))
    ref = dg * gelu_slope64(xd)
    return ref, dg.abs() * gelu_slope_err(xd) + (U + R8) * ref.abs() + TINY


K_ALPHA = torch.tensor(0.70710678118654752440, dtype=F32)
K_BETA = torch.tensor(1.12837916709551257390, dtype=F32) * K_ALPHA * 0.5


def emul_gelu_val(x):
    """fp32 0.5 x (1 + erf(x / sqrt 2)) in the code's order."""
    return 0.5 * x * (1.0 + torch.erf(x * K_ALPHA))


def emul_gelu_slope(x, no_xpdf=False):
    cdf = 0.5 * (1.0 + torch.erf(x * K_ALPHA))
    return cdf if no_xpdf else cdf + x * (torch.exp(-0.5 * x * x) * K_BETA)


def emul_geludrop_fwd(u, p, seed, round_after=False):
    """v bf16. round_after: bf16(gelu_f32 * scale), the value not rounded before the scaling."""
    keep = keep_mask(u.shape, p, seed)
    gf = emul_gelu_val(u.float())
    if p == 0.0:
        return gf.to(BF)
    scale = torch.tensor(drop_scale(p), dtype=F32)
    v = ((gf if round_after else gf.to(BF).float()) * scale).to(BF)
    return torch.where(keep, v, torch.zeros_like(v))


def emul_geludrop_bwd(u, dv, p, seed, no_xpdf=False):
    keep = keep_mask(u.shape, p, seed)
    dg = dv.float()
    if p > 0.0:
        dg = (dg * torch.tensor(drop_scale(p), dtype=F32)).to(BF).float()
        dg = torch.where(keep, dg, torch.zeros_like(dg))
    return (dg * emul_gelu_slope(u.float(), no_xpdf)).to(BF)


# ---- seeded cases (CPU), shared by the GPU and the CPU tests ------------------------------------------

SPECIAL_ROWS = {"mean100": 0, "tiny": 1, "const": 2}   # rows of a case with D = 768, M >= 4
CONST = 2.5     # every partial sum of 768 of them is exact in fp32
EPS = 1e-5
FWD_DS = (256, 512, 768, 1024)
FWD_MS = (1, 3, 4, 5, 9, 130)
BWD_BIG = ((4101, 256), (8197, 256), (4101, 1024))   # second trip partial; third trip partial; NB = 4
FWD_PS = (0.0, 0.1, 0.5)
SEED_HI = 0x9E3779B1   # >= 2^31


def postln_case(M, D):
    """res fp32, y bf16, w around 1 with both signs, b, dh fp32, dhb bf16. At D = 768 and M >= 4 rows
    0 .. 2 are: mean 100 / sigma 0.1 with y = k / 16 (res + yd exact in fp32), mean 0 / sigma 1e-4
    (variance far below eps) with y = 0, and a constant row with y = 0."""
    g = _gen(7, M, D)
    res = torch.randn(M, D, generator=g) * 1.5 + 0.3
    y = torch.randn(M, D, generator=g)
    if D == 768 and M >= 4:
        res[0] = 100.0 + 0.1 * torch.randn(D, generator=g)
        y[0] = torch.randint(-8, 9, (D,), generator=g).float() / 16
        res[1] = 1e-4 * torch.randn(D, generator=g)
        res[2] = CONST
        y[1:3] = 0
    w = (1.0 + 0.25 * torch.randn(D, generator=g)) * (1 - 2 * torch.randint(0, 2, (D,), generator=g)).float()
    b = 0.3 * torch.randn(D, generator=g)
    dh = torch.randn(M, D, generator=g)
    dhb = torch.randn(M, D, generator=g).to(BF)
    return dict(res=res, y=y.to(BF), w=w, b=b, dh=dh, dhb=dhb)


def gelu_case(n, tag=0):
    g = _gen(8, n, tag)
    return (2 * torch.randn(n, generator=g)).to(BF), torch.randn(n, generator=g).to(BF)
