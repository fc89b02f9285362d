// fp32-accurate similarity head on the bf16 MFMA (the `precision="fp32"` mode of the contrastive
// head, model.py:483-488 / 603-608: the reference's use_amp=False sims run with autocast off).
//
// Split-bf16 arithmetic: every fp32 operand x is held as hi = bf16(x), lo = bf16(x - hi), and a
// product of two fp32 operands a . b is formed as  a_lo b_hi + a_hi b_lo + a_hi b_hi  on
// v_mfma_f32_32x32x16_bf16, all three terms into ONE fp32 accumulator, the small terms first (the
// lo . lo term, ~2^-16 of the product, is dropped). gfx950 has no fp32-input MFMA near this rate.
//
//   triad_split_pack          fp32 (B, N, 512) -> the zero-padded hi / lo bf16 operands
//   triad_pairsim_fwd_split   rowmax / argmax / l_nonneg partials / diagonal S (triad_pairsim_fwd
//                             without dS), S in registers only
//   triad_pairsim_dS_split    recompute S, full dS in fp32 registers (as triad_pairsim_dS), stored
//                             as dS_hi + dS_lo in the tiled layout of bwd_gemm.hip
//
// Tiling: a workgroup owns 256 query rows (the decomposition of triad_pairsim_nparts) and has four
// waves, one per SIMD: a wave holds the hi AND lo fragments of 32 query rows (256 VGPRs) and walks
// its two 32-row groups one after the other. Key tiles (32 keys x 512, hi and lo: 64 KB) go
// global -> registers -> LDS into two buffers: the loads of tile b + 1 are issued before the MFMA
// chain of tile b and written to the other buffer after it, one barrier per tile. Plain loads and
// compiler-counted waits only; no atomics (fixed summation order: bit-reproducible).
#include "common.h"

namespace {

constexpr int D = 512;
constexpr int NS = D / 16;            // MFMA k-steps per key tile
constexpr int WAVES = 4;              // 256-thread workgroup, one wave per SIMD (512 registers each)
constexpr int THREADS = 64 * WAVES;
constexpr int ROWS_PER_WG = 256;      // as pairsim_fwd.hip: two 32-row groups per wave
constexpr int GROUPS = ROWS_PER_WG / (32 * WAVES);
constexpr int KT_ELEMS = 32 * D;      // one key tile of one operand in LDS (bf16 elements)
constexpr int STAGE_ELEMS = 2 * KT_ELEMS;   // hi tile then lo tile
constexpr int PIECES = KT_ELEMS / 8 / THREADS;  // 16-byte chunks per thread per operand tile

struct SplitArgs {
  const bf16 *Qhi, *Qlo, *Khi, *Klo;
  int R, R_pad, Nq, Bq, Bk, Nk_pad, Nk_eff, j_per_wg;
  int diag, diag_off;
  const float* temp;
  float clamp_lo;
  float* rowmax;
  int* argmax;         // forward: output; dS: input
  double* part;        // per-workgroup partial (l_nonneg sum in the forward, dtemp in dS)
  float* diagS;
  const float *dclip, *qw, *dSdiag, *coef;
  bf16 *dShi, *dSlo;
  long long CT;
};

struct TileRegs {
  bf16x8 hi[PIECES], lo[PIECES];
};

// Key rows row0 .. row0 + 31 of both operands into registers: chunk idx = u * 256 + tid is chunk
// idx & 63 of row idx >> 6 (a wave reads one whole 1 KB row per instruction).
__device__ __forceinline__ void load_tile(const SplitArgs& a, TileRegs& r, long long row0, int tid) {
#pragma unroll
  for (int u = 0; u < PIECES; ++u) {
    const int idx = u * THREADS + tid;
    const long long off = (row0 + (idx >> 6)) * D + (idx & 63) * 8;
    r.hi[u] = *(const bf16x8*)(a.Khi + off);
    r.lo[u] = *(const bf16x8*)(a.Klo + off);
  }
}

// ... and into one LDS stage: chunk c of row t at chunk c ^ (t & 15) (the swizzle of pairsim.hip's
// stage_key_tile: the ds_read_b128 of 32 rows at one chunk is conflict-free; a wave writes one
// whole row, a permutation of its 64 chunks).
__device__ __forceinline__ void store_tile_lds(bf16* dst, const TileRegs& r, int tid) {
#pragma unroll
  for (int u = 0; u < PIECES; ++u) {
    const int idx = u * THREADS + tid;
    const int t = idx >> 6, c = idx & 63;
    const int p = t * D + ((c ^ (t & 15)) * 8);
    *(bf16x8*)(dst + p) = r.hi[u];
    *(bf16x8*)(dst + KT_ELEMS + p) = r.lo[u];
  }
}

// S^T tile = K_tile . Q_rows^T (the query on the lane, 32 keys in the accumulator, as pairsim.hip),
// three terms into one accumulator, small terms first. kt: this lane's key row of the stage.
__device__ __forceinline__ f32x16 s_tile(const bf16* kt, const bf16x8 (&qhi)[NS], const bf16x8 (&qlo)[NS],
                                         const int (&koff)[8]) {
  f32x16 acc = {};
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int o = koff[s & 7] + (s >> 3) * 128;
    const bf16x8 khi = *(const bf16x8*)(kt + o);
    const bf16x8 klo = *(const bf16x8*)(kt + KT_ELEMS + o);
    acc = mfma32(khi, qlo[s], acc);
    acc = mfma32(klo, qhi[s], acc);
    if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // keep the LDS reads near their MFMAs (register budget)
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const bf16x8 khi = *(const bf16x8*)(kt + koff[s & 7] + (s >> 3) * 128);
    acc = mfma32(khi, qhi[s], acc);
    if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
  }
  return acc;
}

// Store a wave's 32 x 32 tile of dS as hi + lo (accumulator order, chunks in ds_chunk order).
__device__ __forceinline__ void store_tile_split(bf16* dShi, bf16* dSlo, long long CT, int rt, long long ct,
                                                 int lane, const float (&g)[16]) {
  const long long o = ((long long)rt * CT + ct) * 1024 + lane * 8;
  bf16x8 ha, hb, la, lb;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const bf16 h0 = (bf16)g[k], h1 = (bf16)g[8 + k];
    ha[k] = h0;
    hb[k] = h1;
    la[k] = (bf16)(g[k] - (float)h0);
    lb[k] = (bf16)(g[8 + k] - (float)h1);
  }
  *(bf16x8*)(dShi + o) = ha;
  *(bf16x8*)(dShi + o + 512) = hb;
  *(bf16x8*)(dSlo + o) = la;
  *(bf16x8*)(dSlo + o + 512) = lb;
}

// DS = false: the forward (rowmax, first argmax, l_nonneg partial, diagonal S).
// DS = true:  the recompute backward's dS (hi + lo) and dL/dtemp partial.
template <bool DS>
__global__ __launch_bounds__(THREADS, 1) void pairsim_split_kernel(SplitArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 kbuf[2 * STAGE_ELEMS + 4 * WAVES];
  double* red = (double*)(kbuf + 2 * STAGE_ELEMS);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, ql = lane & 31;

  int koff[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) koff[k] = ((2 * k + h) ^ (ql & 15)) * 8;

  const int j0 = blockIdx.y * a.j_per_wg;
  const int j1 = min(a.Bk, j0 + a.j_per_wg);
  const int nkb = a.Nk_pad / 32;
  const int nblocks = (j1 - j0) * nkb;
  const int pidx = blockIdx.y * gridDim.x + blockIdx.x;
  if (nblocks <= 0) {  // uniform across the workgroup
    if (tid == 0) a.part[pidx] = 0.0;
    return;
  }
  const float temp = *a.temp;
  const float lo = a.clamp_lo;
  float c_ce = 0.f, c_nn = 0.f, c_dg = 0.f;
  if (DS) { c_ce = a.coef[0]; c_nn = a.coef[1]; c_dg = a.coef[2]; }
  const long long krow0 = (long long)j0 * a.Nk_pad;

  double accd = 0.0;
  for (int grp = 0; grp < GROUPS; ++grp) {
    const int row = blockIdx.x * ROWS_PER_WG + (grp * WAVES + wave) * 32 + ql;
    const bool row_ok = row < a.R;
    const int qi = row_ok ? row / a.Nq : -1;
    const int qq = row_ok ? row - qi * a.Nq : 0;
    const int rt = blockIdx.x * (ROWS_PER_WG / 32) + grp * WAVES + wave;  // this wave's row tile of dS

    // Query fragments: lane holds Q[row][16 s + 8 h .. +8] for s = 0..31 (the B operand).
    bf16x8 qhi[NS], qlo[NS];
    {
      const size_t qo = (size_t)row * D + 8 * h;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        qhi[s] = *(const bf16x8*)(a.Qhi + qo + 16 * s);
        qlo[s] = *(const bf16x8*)(a.Qlo + qo + 16 * s);
      }
    }
    const float wrow = (DS && row_ok) ? a.qw[row] : 0.f;

    TileRegs tr;
    load_tile(a, tr, krow0, tid);
    store_tile_lds(kbuf, tr, tid);   // every wave left both stages behind the previous group's last barrier
    __syncthreads();

    float rm = -INFINITY, gmax = 0.f;
    int ra = -1;
    for (int b = 0; b < nblocks; ++b) {
      const int j = j0 + b / nkb, kb = b - (b / nkb) * nkb;
      if (b + 1 < nblocks) load_tile(a, tr, krow0 + (long long)(b + 1) * 32, tid);
      const f32x16 acc = s_tile(kbuf + (b & 1) * STAGE_ELEMS + ql * D, qhi, qlo, koff);

      const bool diag_pair = a.diag && row_ok && (j == qi + a.diag_off);
      const int key0 = kb * 32 + 4 * h;
      if (!DS) {
        if (kb == 0) { rm = -INFINITY; ra = -1; }
        float* dp = (diag_pair && a.diagS) ? a.diagS + ((size_t)qi * a.Nq + qq) * a.Nk_pad : nullptr;
        float m = -INFINITY, nn = 0.f;
        int mi = -1;
#pragma unroll
        for (int v = 0; v < 16; ++v) {   // keys ascend with v: a strict > keeps the first argmax
          const int key = key0 + (v & 3) + 8 * (v >> 2);
          const float s = acc[v] * temp;
          if (key < a.Nk_eff) {
            const float c = fminf(fmaxf(s, lo), 0.f);
            nn += c * c;
            if (s > m) { m = s; mi = key; }
          }
          if (dp) dp[key] = s;
        }
        if (row_ok) accd += (double)nn;
        const float om = __shfl_xor(m, 32);
        const int oi = __shfl_xor(mi, 32);
        if (om > m || (om == m && oi >= 0 && oi < mi)) { m = om; mi = oi; }
        if (m > rm) { rm = m; ra = mi; }   // later tiles hold larger keys: ties keep the earlier
        if (kb == nkb - 1 && h == 0) {
          a.rowmax[(size_t)j * a.R_pad + row] = rm;
          a.argmax[(size_t)j * a.R_pad + row] = ra;
        }
      } else {
        if (kb == 0) {
          gmax = row_ok ? c_ce * a.dclip[(size_t)qi * a.Bk + j] * wrow : 0.f;
          ra = row_ok ? a.argmax[(size_t)j * a.R_pad + row] : -1;
        }
        const float* dg = (diag_pair && a.dSdiag) ? a.dSdiag + ((size_t)qi * a.Nq + qq) * a.Nk_pad : nullptr;
        float dt = 0.f;
        float out[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int key = key0 + (v & 3) + 8 * (v >> 2);
          const float sraw = acc[v];
          const float s = sraw * temp;
          float g = (s >= lo && s <= 0.f) ? c_nn * s : 0.f;  // clamp grad, inclusive bounds
          if (key == ra) g += gmax;
          if (dg && key < a.Nk_eff) g += c_dg * dg[key];
          g = (row_ok && key < a.Nk_eff) ? g : 0.f;
          dt += g * sraw;
          out[v] = g;
        }
        accd += (double)dt;
        store_tile_split(a.dShi, a.dSlo, a.CT, rt, (long long)j * nkb + kb, lane, out);
      }

      if (b + 1 < nblocks) store_tile_lds(kbuf + ((b + 1) & 1) * STAGE_ELEMS, tr, tid);
      __syncthreads();  // tile b + 1 is in LDS; every wave is done with stage b & 1
    }
  }

  // Workgroup partial, in double, in a fixed order.
  const double v = wave_sum_d(accd);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < WAVES; ++w) t += red[w];
    a.part[pidx] = t;
  }
}

// fp32 rows -> hi / lo bf16 rows; one thread per 8 features. Output row o holds sample o / N_pad's
// token o % N_pad when that is < N and the sample < B, else zeros.
__global__ __launch_bounds__(256) void split_pack_kernel(const float* __restrict__ x, int B, int N, int N_pad,
                                                         long long rows_alloc, bf16* __restrict__ hi,
                                                         bf16* __restrict__ lo) {
  const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long o = e >> 6;
  if (o >= rows_alloc) return;
  const int c = (int)(e & 63) * 8;
  const long long b = o / N_pad;
  const int t = (int)(o - b * N_pad);
  bf16x8 vh = {}, vl = {};
  if (b < B && t < N) {
    const float* src = x + ((size_t)b * N + t) * D + c;
    const f32x4 f0 = *(const f32x4*)src, f1 = *(const f32x4*)(src + 4);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float f = k < 4 ? f0[k] : f1[k - 4];
      const bf16 hv = (bf16)f;
      vh[k] = hv;
      vl[k] = (bf16)(f - (float)hv);
    }
  }
  *(bf16x8*)(hi + o * D + c) = vh;
  *(bf16x8*)(lo + o * D + c) = vl;
}

bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

int check_split(const void* Qhi, const void* Qlo, const void* Khi, const void* Klo, int R, int R_pad, int Nq, int Bq,
                int Bk, int Nk_pad, int Nk_eff, int D_, const float* temp) {
  if (!Qhi || !Qlo || !Khi || !Klo || !temp) return TRIAD_EINVAL;
  if (misaligned(Qhi) || misaligned(Qlo) || misaligned(Khi) || misaligned(Klo)) return TRIAD_EINVAL;
  if (D_ != D || R_pad <= 0 || R_pad % ROWS_PER_WG || R > R_pad || R <= 0 || Nq <= 0 || Bq <= 0 || Bk <= 0 ||
      Nk_pad <= 0 || Nk_pad % 32 || Nk_eff <= 0 || Nk_eff > Nk_pad)
    return TRIAD_EINVAL;
  return TRIAD_OK;
}

void fill(SplitArgs& a, const void* Qhi, const void* Qlo, const void* Khi, const void* Klo, int R, int R_pad, int Nq,
          int Bq, int Bk, int Nk_pad, int Nk_eff, const float* temp, float clamp_lo, int diag, int diag_off,
          dim3* grid) {
  a.Qhi = (const bf16*)Qhi; a.Qlo = (const bf16*)Qlo; a.Khi = (const bf16*)Khi; a.Klo = (const bf16*)Klo;
  a.R = R; a.R_pad = R_pad; a.Nq = Nq; a.Bq = Bq; a.Bk = Bk; a.Nk_pad = Nk_pad; a.Nk_eff = Nk_eff;
  a.diag = diag; a.diag_off = diag_off; a.temp = temp; a.clamp_lo = clamp_lo;
  // the key-sample split of triad_pairsim_fwd / _dS (pairsim.hip grid_for), whose split count is a
  // fixed point of ys -> ceil(Bk / ceil(Bk / ys)): recovered from the partial count it reports
  const int xb = R_pad / ROWS_PER_WG;
  const int ys = triad_pairsim_nparts(R_pad, Bk) / xb;
  a.j_per_wg = (Bk + ys - 1) / ys;
  *grid = dim3(xb, ys);
}

}  // namespace

extern "C" {

int triad_split_pack(const float* x, int B, int N, int N_pad, long long rows_alloc, void* hi, void* lo,
                     hipStream_t stream) {
  if (!x || !hi || !lo || misaligned(x) || misaligned(hi) || misaligned(lo)) return TRIAD_EINVAL;
  if (B <= 0 || N <= 0 || N_pad < N || rows_alloc < (long long)B * N_pad) return TRIAD_EINVAL;
  const long long blocks = (rows_alloc * 64 + 255) / 256;
  if (blocks > 0x7fffffffLL) return TRIAD_EINVAL;
  hipLaunchKernelGGL(split_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, B, N, N_pad, rows_alloc,
                     (bf16*)hi, (bf16*)lo);
  TRIAD_CHECK_LAUNCH();
  return TRIAD_OK;
}

int triad_pairsim_fwd_split(const void* Qhi, const void* Qlo, const void* Khi, const void* Klo, int R, int R_pad,
                            int Nq, int Bq, int Bk, int Nk_pad, int Nk_eff, int D_, const float* temp,
                            float clamp_lo, int diag, int diag_off, float* rowmax, int* argmax, double* nn_part,
                            float* diagS, hipStream_t stream) {
  if (int e = check_split(Qhi, Qlo, Khi, Klo, R, R_pad, Nq, Bq, Bk, Nk_pad, Nk_eff, D_, temp)) return e;
  if (!rowmax || !argmax || !nn_part) return TRIAD_EINVAL;
  if (diag && diagS && (diag_off < 0 || diag_off + Bq > Bk)) return TRIAD_EINVAL;
  SplitArgs a = {};
  dim3 grid;
  fill(a, Qhi, Qlo, Khi, Klo, R, R_pad, Nq, Bq, Bk, Nk_pad, Nk_eff, temp, clamp_lo, diag, diag_off, &grid);
  a.rowmax = rowmax; a.argmax = argmax; a.part = nn_part; a.diagS = diagS;
  hipLaunchKernelGGL(pairsim_split_kernel<false>, grid, dim3(THREADS), 0, stream, a);
  TRIAD_CHECK_LAUNCH();
  return TRIAD_OK;
}

int triad_pairsim_dS_split(const void* Qhi, const void* Qlo, const void* Khi, const void* Klo, int R, int R_pad,
                           int Nq, int Bq, int Bk, int Nk_pad, int Nk_eff, int D_, const float* temp, float clamp_lo,
                           int diag, int diag_off, const int* argmax, const float* dclip, const float* qw,
                           const float* dSdiag, const float* coef, void* dS_hi, void* dS_lo, long long CT,
                           double* dt_part, hipStream_t stream) {
  if (int e = check_split(Qhi, Qlo, Khi, Klo, R, R_pad, Nq, Bq, Bk, Nk_pad, Nk_eff, D_, temp)) return e;
  if (!argmax || !dclip || !qw || !coef || !dS_hi || !dS_lo || !dt_part) return TRIAD_EINVAL;
  if (misaligned(dS_hi) || misaligned(dS_lo)) return TRIAD_EINVAL;
  if (CT <= 0 || CT % 4 || CT * 32 < (long long)Bk * Nk_pad) return TRIAD_EINVAL;
  SplitArgs a = {};
  dim3 grid;
  fill(a, Qhi, Qlo, Khi, Klo, R, R_pad, Nq, Bq, Bk, Nk_pad, Nk_eff, temp, clamp_lo, diag, diag_off, &grid);
  a.argmax = (int*)argmax; a.dclip = dclip; a.qw = qw; a.dSdiag = dSdiag; a.coef = coef;
  a.dShi = (bf16*)dS_hi; a.dSlo = (bf16*)dS_lo; a.CT = CT; a.part = dt_part;
  hipLaunchKernelGGL(pairsim_split_kernel<true>, grid, dim3(THREADS), 0, stream, a);
  TRIAD_CHECK_LAUNCH();
  return TRIAD_OK;
}

}  // extern "C"
