// bf16 MFMA GEMMs for the backward of the fused similarity head:
//   dQ[r][d] = temp * sum_c dS[r][c] * K[c][d]      (A = dS,   k-contiguous)
//   dK[c][d] = temp * sum_r dS[r][c] * Q[r][d]      (A = dS^T, read transposed from dS)
// i.e. the gradients of S = temp * Q K^T (model.py:387 / 505) w.r.t. both operands.
// B (= K or Q, [k][n] row-major, n-contiguous) is always read with the gfx950
// transposing LDS read ds_read_b64_tr_b16, so neither dS nor the features are
// ever copied into a transposed layout in HBM.
//
// Tile 128x128x64, 4 waves (2x2), each wave 64x64 = 2x2 tiles of
// v_mfma_f32_32x32x16_bf16. Operands are staged global->LDS with 16-byte LDS-DMA
// (global_load_lds_dwordx4) into two buffers; swizzles are applied on the
// global SOURCE address so the lane-linear DMA image is bank-conflict-free for
// the reads (ds_read_b128 for k-contiguous, ds_read_b64_tr_b16 for the others).
#include "common.h"

#include <atomic>
#include <type_traits>

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int A_ELEMS = BM * BK, B_ELEMS = BK * BN;

// k-contiguous image [m][64 k] (128-B rows): 16-B chunk c of row m lives at chunk c ^ ((m >> 1) & 7)
__device__ __forceinline__ int kc_off(int m, int chunk) { return m * BK + ((chunk ^ ((m >> 1) & 7)) << 3); }
// n-contiguous image [k][128 n] (256-B rows): chunk c of row k lives at chunk c ^ ((k & 3) << 2)
__device__ __forceinline__ int nc_off(int k, int col) {
  return k * BN + ((((col >> 3) ^ ((k & 3) << 2))) << 3) + (col & 7);
}

// piece u (0..3) of this wave's share of an A stage (one 16-byte LDS-DMA wave-instruction)
template <bool A_KCONTIG>
__device__ __forceinline__ void stage_a_piece(const bf16* __restrict__ A, long long lda, int m0, int k0, bf16* dst,
                                              int wave, int lane, int u) {
  const int inst = wave * 4 + u;
  if (A_KCONTIG) {  // 16 wave-instructions of 8 rows x 128 B
    const int m = inst * 8 + (lane >> 3), cp = lane & 7;
    const int c = cp ^ ((m >> 1) & 7);
    glds16(A + (size_t)(m0 + m) * lda + k0 + c * 8, dst + inst * 512);
  } else {  // A stored [k][m]: 16 wave-instructions of 4 k-rows x 256 B
    const int k = inst * 4 + (lane >> 4), cp = lane & 15;
    const int c = cp ^ ((k & 3) << 2);
    glds16(A + (size_t)(k0 + k) * lda + m0 + c * 8, dst + inst * 512);
  }
}

template <bool A_KCONTIG>
__device__ __forceinline__ void stage_a(const bf16* __restrict__ A, long long lda, int m0, int k0, bf16* dst,
                                        int wave, int lane) {
#pragma unroll
  for (int u = 0; u < 4; ++u) stage_a_piece<A_KCONTIG>(A, lda, m0, k0, dst, wave, lane, u);
}

// (Measured and not kept: staging through VGPRs + ds_write instead of LDS-DMA, and the next
// stage's DMA pieces spread between the MFMAs -- DESIGN.md §4b.)

// B is [k][n] (B_KCONTIG=0, n-contiguous) or [n][k] (B_KCONTIG=1) -- the same two
// images as A with the roles of m and n swapped.
template <bool B_KCONTIG>
__device__ __forceinline__ void stage_b(const bf16* __restrict__ B, long long ldb, int n0, int k0, bf16* dst,
                                        int wave, int lane) {
  stage_a<B_KCONTIG>(B, ldb, n0, k0, dst, wave, lane);
}

// Fragment of a [k][n]-image operand for MFMA 32x32x16: lane l needs
// X[k = 16 s + 8 h + j][n = n0 + (l & 31)], j = 0..7, via two 4-row transposed reads.
__device__ __forceinline__ bf16x8 frag_tr(const bf16* img, int n0, int s, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3, hh = g >> 1;
  const int col = n0 + 16 * (g & 1) + 4 * p;
  const int k0 = 16 * s + 8 * hh + q;
  const s16x4 lo = lds_tr16(img + nc_off(k0, col));
  const s16x4 hi = lds_tr16(img + nc_off(k0 + 4, col));
  bf16x8 r;
  s16x4* rp = (s16x4*)&r;
  rp[0] = lo;
  rp[1] = hi;
  return r;
}

// F.linear's bias for output column n, added before the one rounding: fp32, or bf16 as the
// autocast model holds it (read as is, no fp32 copy of the vector per call)
__device__ __forceinline__ float bias_at(const void* bias, int bias_bf16, int n) {
  if (!bias) return 0.f;
  return bias_bf16 ? (float)((const bf16*)bias)[n] : ((const float*)bias)[n];
}

// Workgroup -> (output tile, k split). Default: XCD-aware bijective remap of blockIdx.x -- blocks
// sharing an XCD (bid % 8 under round-robin placement) get consecutive tiles, so the column tiles
// of one row panel of A share that XCD's L2; blockIdx.y is the split. xsplit (split-K weight
// gradients, gridDim.y % 8 == 0): every tile of one split on ONE XCD instead, so that split's
// token slab of both operands is fetched from HBM once, into that XCD's L2, and read from there
// by all its tiles (the default mapping puts each split's tiles on all eight XCDs: each operand
// slab is fetched up to 8 times). Placement is a speed matter only; results do not depend on it.
__device__ __forceinline__ int xcd_tile(int bid, int T) {
  const int q8 = T / 8, r8 = T % 8, x = bid % 8;
  return (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + bid / 8;
}

__device__ __forceinline__ void tile_split(int xsplit, int& tile, int& split) {
  const int T = gridDim.x;
  if (xsplit) {
    const int L = blockIdx.y * T + blockIdx.x, c = L % 8, i = L / 8;
    tile = i % T;
    split = c + 8 * (i / T);
    return;
  }
  tile = xcd_tile(blockIdx.x, T);
  split = blockIdx.y;
}

template <bool A_KCONTIG, bool B_KCONTIG, typename OutT>
__global__ __launch_bounds__(256, 2) void gemm_kernel(const bf16* __restrict__ A, long long lda,
                                                      const bf16* __restrict__ B, long long ldb,
                                                      int M, int N, int Kd, const float* __restrict__ alpha_p,
                                                      OutT* __restrict__ C, long long ldc, int k_per_split,
                                                      long long slab_stride, const void* __restrict__ bias, int bias_bf16, int xsplit) {
  __shared__ __attribute__((aligned(16))) bf16 lds[2 * (A_ELEMS + B_ELEMS)];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5;

  int swz, split;
  tile_split(xsplit, swz, split);
  const int ntn = N / BN;
  const int m0 = (swz / ntn) * BM, n0 = (swz % ntn) * BN;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f32x16){};

  // split-K: split owns k in [kbeg, kbeg + k_per_split) and writes its own slab of C
  const int kbeg = split * k_per_split;
  const int nk = min(k_per_split, Kd - kbeg) / BK;
  C += (size_t)split * slab_stride;
  if (nk > 0) {
    stage_a<A_KCONTIG>(A, lda, m0, kbeg, lds, wave, lane);
    stage_b<B_KCONTIG>(B, ldb, n0, kbeg, lds + A_ELEMS, wave, lane);
  }
  for (int kt = 0; kt < nk; ++kt) {
    lds_dma_barrier();
    bf16* const nb = lds + ((kt + 1) & 1) * (A_ELEMS + B_ELEMS);
    const bool pf = kt + 1 < nk;
    if (pf) {
      stage_a<A_KCONTIG>(A, lda, m0, kbeg + (kt + 1) * BK, nb, wave, lane);
      stage_b<B_KCONTIG>(B, ldb, n0, kbeg + (kt + 1) * BK, nb + A_ELEMS, wave, lane);
    }
    const bf16* ai = lds + (kt & 1) * (A_ELEMS + B_ELEMS);
    const bf16* bi = ai + A_ELEMS;
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      bf16x8 af[2], bfr[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int mrow = wm * 64 + t * 32;
        if (A_KCONTIG) {
          af[t] = *(const bf16x8*)(ai + kc_off(mrow + (lane & 31), 2 * s + h));
        } else {
          // A image is [k][m] (256-B rows, same layout as B's)
          af[t] = frag_tr(ai, mrow, s, lane);
        }
        const int ncol = wn * 64 + t * 32;
        if (B_KCONTIG) {
          bfr[t] = *(const bf16x8*)(bi + kc_off(ncol + (lane & 31), 2 * s + h));
        } else {
          bfr[t] = frag_tr(bi, ncol, s, lane);
        }
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          acc[a][b] = mfma32(af[a], bfr[b], acc[a][b]);
        }
    }
  }

  const float alpha = alpha_p ? *alpha_p : 1.f;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int n = n0 + wn * 64 + b * 32 + (lane & 31);
      const float bn = bias_at(bias, bias_bf16, n);   // F.linear's bias, added before the one rounding
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int m = m0 + wm * 64 + a * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
        C[(size_t)m * ldc + n] = (OutT)(alpha * acc[a][b][v] + bn);
      }
    }
}

// ---- 256 x 128 ring form ----------------------------------------------------------------------
// Workgroup = 8 waves (4 x 2, each 64 x 64 as above), tile 256 (M) x 128 (N) x 64 (K) per stage,
// a 3-slot LDS ring (3 x 48 KB) with the next-but-one stage's LDS-DMA issued while the current
// one computes; each wave issues exactly 6 pieces per stage, so the wait for stage kt is a
// counted `s_waitcnt vmcnt(6)` (stage kt+1 stays in flight) + the barrier. Twice the B reuse
// of the 128 x 128 form. The A image is [256][64] (k-contiguous A) or two [64][128] halves.
constexpr int GB_M = 256, GB_NB = 3;
constexpr int GB_A = GB_M * BK, GB_ST = GB_A + B_ELEMS;  // elements per stage (48 KB)
constexpr int GB_PIECES = 6;

// the 6 DMA pieces of a stage issued between its 16 MFMAs (one per 2), not in a burst (measured)

template <bool A_KCONTIG, bool B_KCONTIG>
__device__ __forceinline__ void gb_piece(const bf16* __restrict__ A, long long lda, const bf16* __restrict__ B,
                                         long long ldb, int m0, int n0, int k0, bf16* dst, int wave, int lane,
                                         int u) {
  if (u < 4) {  // A: 32 pieces, 4 per wave
    const int inst = wave * 4 + u;
    if (A_KCONTIG) {  // 8 rows x 128 B
      const int m = inst * 8 + (lane >> 3), cp = lane & 7;
      const int c = cp ^ ((m >> 1) & 7);
      glds16(A + (size_t)(m0 + m) * lda + k0 + c * 8, dst + inst * 512);
    } else {  // half inst >> 4, 4 k-rows x 256 B
      const int half = inst >> 4, ii = inst & 15;
      const int k = ii * 4 + (lane >> 4), cp = lane & 15;
      const int c = cp ^ ((k & 3) << 2);
      glds16(A + (size_t)(k0 + k) * lda + m0 + half * 128 + c * 8, dst + half * (BK * 128) + ii * 512);
    }
  } else {  // B: 16 pieces, 2 per wave
    const int inst = wave * 2 + (u - 4);
    bf16* bd = dst + GB_A;
    if (B_KCONTIG) {
      const int n = inst * 8 + (lane >> 3), cp = lane & 7;
      const int c = cp ^ ((n >> 1) & 7);
      glds16(B + (size_t)(n0 + n) * ldb + k0 + c * 8, bd + inst * 512);
    } else {
      const int k = inst * 4 + (lane >> 4), cp = lane & 15;
      const int c = cp ^ ((k & 3) << 2);
      glds16(B + (size_t)(k0 + k) * ldb + n0 + c * 8, bd + inst * 512);
    }
  }
}

template <bool A_KCONTIG, bool B_KCONTIG, typename OutT>
__global__ __launch_bounds__(512, 1) void gemm_big_kernel(const bf16* __restrict__ A, long long lda,
                                                          const bf16* __restrict__ B, long long ldb, int M, int N,
                                                          int Kd, const float* __restrict__ alpha_p,
                                                          OutT* __restrict__ C, long long ldc, int k_per_split,
                                                          long long slab_stride, const void* __restrict__ bias, int bias_bf16, int xsplit) {
  __shared__ __attribute__((aligned(16))) bf16 lds[GB_NB * GB_ST];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5;
  int swz, split;
  tile_split(xsplit, swz, split);
  const int ntn = N / BN;
  const int m0 = (swz / ntn) * GB_M, n0 = (swz % ntn) * BN;

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f32x16){};

  const int kbeg = split * k_per_split;
  const int nk = __builtin_amdgcn_readfirstlane(max(0, min(k_per_split, Kd - kbeg)) / BK);
  C += (size_t)split * slab_stride;
#pragma unroll
  for (int p = 0; p < GB_NB - 1; ++p)
    if (p < nk)
#pragma unroll
      for (int u = 0; u < GB_PIECES; ++u)
        gb_piece<A_KCONTIG, B_KCONTIG>(A, lda, B, ldb, m0, n0, kbeg + p * BK, lds + p * GB_ST, wave, lane, u);
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) TRIAD_VMCNT(GB_PIECES);
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const bool pf = kt + GB_NB - 1 < nk;
    bf16* const nb = lds + ((kt + GB_NB - 1) % GB_NB) * GB_ST;
    const int kn = kbeg + (kt + GB_NB - 1) * BK;
    const bf16* ai = lds + (kt % GB_NB) * GB_ST;
    const bf16* bi = ai + GB_A;
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      bf16x8 af[2], bfr[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int mrow = wm * 64 + t * 32;
        if (A_KCONTIG) af[t] = *(const bf16x8*)(ai + kc_off(mrow + (lane & 31), 2 * s + h));
        else af[t] = frag_tr(ai + (mrow >> 7) * (BK * 128), mrow & 127, s, lane);
        const int ncol = wn * 64 + t * 32;
        if (B_KCONTIG) bfr[t] = *(const bf16x8*)(bi + kc_off(ncol + (lane & 31), 2 * s + h));
        else bfr[t] = frag_tr(bi, ncol, s, lane);
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          acc[a][b] = mfma32(af[a], bfr[b], acc[a][b]);
          const int mi = s * 4 + a * 2 + b;
          if ((mi & 1) && mi / 2 < GB_PIECES) {
            __builtin_amdgcn_sched_barrier(0);
            if (pf) gb_piece<A_KCONTIG, B_KCONTIG>(A, lda, B, ldb, m0, n0, kn, nb, wave, lane, mi / 2);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
    }
  }

  const float alpha = alpha_p ? *alpha_p : 1.f;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int n = n0 + wn * 64 + b * 32 + (lane & 31);
      const float bn = bias_at(bias, bias_bf16, n);   // F.linear's bias, added before the one rounding
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int m = m0 + wm * 64 + a * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
        C[(size_t)m * ldc + n] = (OutT)(alpha * acc[a][b][v] + bn);
      }
    }
}

// ---- 256 x 256 tile: LDS images and staging (the eight-wave form below) -------------------------
// Tile 256 x 256 x 64 per stage, two 64 KB LDS slots. Images (one wave-instruction = 1 KB):
//   k-contiguous X ([rows][k]): [256][64], piece inst = rows 8 inst .. + 7 x 128 B, 16-byte chunk c
//     of row m fetched into chunk c ^ ((m >> 1) & 7) (kc_off);
//   X stored [k][rows]: two [64][128] halves, piece inst = half inst >> 4, k-rows 4 (inst & 15) .. + 3
//     x 256 B, chunk c of row k fetched into chunk c ^ ((k & 3) << 2) (nc_off).
// (Round 1 ran this tile on four waves, 128 x 128 each; measured bounds,
// profiles/r01_gemm_w4_bounds.log: without the fragment reads 3 % faster, without the DMA 25 %
// faster -- the LDS-DMA fill rate (~64 KB per CU per stage) holds it under the MFMA rate. The
// eight-wave form replaced it in round 2, 3-13 % faster; the four-wave kernel was deleted in round 5.)
constexpr int GW_M = 256, GW_N = 256;
constexpr int GW_A = GW_M * BK, GW_ST = GW_A + GW_N * BK;  // elements per stage (64 KB)

template <bool KCONTIG>
__device__ __forceinline__ bf16x8 gw_frag(const bf16* img, int row, int s, int lane) {
  if (KCONTIG) return *(const bf16x8*)(img + kc_off(row + (lane & 31), 2 * s + (lane >> 5)));
  return frag_tr(img + (row >> 7) * (BK * 128), row & 127, s, lane);
}

// ---- 256 x 256 eight-wave form -----------------------------------------------------------------
// The 256 x 256 tile with 8 waves, two per SIMD: wave (wm, wn) of 2 x 4 owns 128 x 64 (4 x 2 tiles
// of 32 x 32, 128 accumulators per lane) and issues 8 of a stage's 64 DMA pieces. Until the
// pipelined loop below, every stage began with vmcnt(0) + __syncthreads() (no DMA in flight across
// a barrier, all eight waves in phase); measured in that drained structure and not kept
// (profiles/r02_gemm_w8_variants_ab.log, 16 c3 shapes): s_setprio(1) around each step's MFMA
// cluster -0.4 %, a static priority for the younger four waves 0.0 %, the next stage's 8 DMA
// pieces in a burst after the barrier +3.9 %, a 4-slot ring of 32-deep chunks +5-8 %.
// Measured in the pipelined structure (tools/gemm_w8_ab.py against the drained loop's build,
// alternated in one process, profiles/gemm_w8_pipe_ab.log; every output bit-equal): the c3 shapes
// weighted by launches -8.1 % (both operands k-contiguous), -7.4 % (input gradients), -12.7 %
// (split-K weight gradients); 3-9 % at K = 768 (12 k-steps), 10-19 % from K = 2304 up. With every
// wave executing the last k-step's trailing barrier and wm = 0 one more (wm = 0 then waits out
// wm = 1's last MFMA cluster before its epilogue) the same sums read -6 / -7 / -10 % and the
// two 8-k-step conv shapes were 10-12 % slower than the drained loop. s_setprio around the MFMA
// clusters is kept as the structure needs it (without the pair hipcc moves MFMAs across the raw
// barriers); it was not measured apart in this structure.
// Epilogue forms measured on the drained loop and not kept: transposed accumulators (B fragment
// first) with 8-byte row-run stores +10 % (profiles/r02_gemm_w8_tepi_ab.log); the bf16 tile staged
// through LDS and stored as 128-B row runs of 16-B stores: equal
// (profiles/r02_gemm_w8_ldsepi_ab.log). A diagnostic build without the epilogue stores ran 10 %
// faster (18 % on the wide K = 768 shapes, profiles/r02_gemm_w8_nostore_diag.log): the cost is the
// output write itself, ~128 KB per workgroup issued by every CU of a dispatch round at once and not
// overlapped with any MFMA work.

// ---- the pipelined main loop: LDS-DMA in flight across raw barriers ------------------------------
// One k-step (a 64-deep stage in slot c = kt & 1) is four phases; phase p is this wave's 8 MFMAs
// on one 64 x 32 quadrant of its 128 x 64 output over the whole stage:
//     fragment reads | one half-tile's 2 DMA pieces | [vmcnt] | lgkmcnt(0) | s_barrier |
//     s_setprio(1), 8 MFMAs, s_setprio(0) | s_barrier
// Quadrants and the fragments a phase reads (kept in registers until their last quadrant):
//     p0: (rows 0-63, cols 0-31)   reads A rows 0-63, B cols 0-31 (and cols 32-63 when B is [k][n])
//     p1: (rows 0-63, cols 32-63)  reads B cols 32-63 (B [n][k] only)
//     p2: (rows 64-127, cols 32-63) reads A rows 64-127
//     p3: (rows 64-127, cols 0-31)  reads nothing
// A stage is four half-tiles of 16 KB = GP_LOADS (2) wave-instructions per wave each. A: pieces
// wave * 4 + u, u in {0, 1} / {2, 3}. B [k][n]: the same. B [n][k]: half hh is the 32-column
// sub-tiles hh of all four wave columns (n = 64 wn + 32 hh + 0..31), so that half 0 is read in p0
// only. Issue order, global phase P = 4 kt + p (stage kt + 1 lives in slot c ^ 1, kt + 2 in c):
//     p0: A half 1 of stage kt + 1      p1: B half 0 of stage kt + 2
//     p2: B half 1 of stage kt + 2      p3: A half 0 of stage kt + 2, then vmcnt(GP_LOADS * GP_FLIGHT)
// Wave rows wm = 1 run one barrier behind wm = 0 (one s_barrier more before their first phase, one
// fewer after their last MFMA cluster: every wave executes 1 + 8 nk barriers), so on every SIMD one
// wave's MFMA cluster runs beside the other's reads and DMA issue. Number the barriers every wave
// executes g = 0, 1, ...: wm = 0 runs the read / issue / wait part of phase P before barrier 2P and
// its MFMAs before 2P + 1; wm = 1 before 2P + 1 and 2P + 2.
//   RAW (LDS-DMA data is ordered for a ds_read only by the issuing wave's vmcnt and a barrier the
//   reader has passed since): p3's vmcnt(6) leaves the three half-tiles issued in p1-p3 (stage
//   kt + 2) in flight and retires everything older, i.e. all of stage kt + 1, in every wave before
//   barrier 2(4 kt + 3) + 1 at the latest (wm = 1). Stage kt + 1 is first read in phase 4 kt + 4:
//   before barrier 2(4 kt + 4) by wm = 0 and a barrier later by wm = 1 -- after that barrier for
//   both. Never in the phase of the wait itself.
//   WAR (a slot half may be restaged one phase after its last read, because every phase retires
//   its reads with lgkmcnt(0) BEFORE its first barrier: reads of phase P are done in every wave at
//   barrier 2P + 1, and the earliest issue of phase P + 1 is wm = 0's, after barrier 2P + 1):
//     B half 0 of slot c: last read p0 (phase 4 kt)      restaged 4 kt + 1
//     B half 1 of slot c: last read p1 (p0 for [k][n])   restaged 4 kt + 2
//     A (both halves) of slot c: last read p2            restaged 4 kt + 3 (half 0), 4 kt + 4 (half 1)
// Prologue: stage 0 and the first three half-tiles of stage 1, vmcnt(6) (vmcnt(0) when nk = 1),
// barrier. The loop body is two steady k-steps (static slots) and runs while three stages remain;
// the last two k-steps run after it: the one before last issues only A half 1 of the last stage
// and drains with vmcnt(0) in its p3, the last issues nothing, so no slot is read unstaged for any
// nk >= 1. Inside the loop no wait is vmcnt(0). (tests/test_gemm_w8_isa_cpu.py re-derives the
// constant from the emitted loop.)
constexpr int GP_LOADS = 2;    // LDS-DMA wave-instructions per wave per half-tile
constexpr int GP_FLIGHT = 3;   // half-tiles left in flight by the steady-state wait
enum { GP_STEADY = 0, GP_PENULT = 1, GP_LAST = 2 };

// One DMA piece of the images above, addressed as a wave-uniform 64-bit base (SGPRs) plus a
// 32-bit per-lane byte offset: the per-lane part of a piece's source address depends only on the
// lane and on the piece's parity (inst & 1 enters the k-contiguous swizzle), so a stage's 8 pieces
// need 4 offset VGPRs in all instead of 8 per-lane 64-bit pointers. The base is computed on the
// scalar unit; s_nop 2 keeps five wait states between any instruction before the statement and
// the load should hipcc ever hand over a base fresh from v_readfirstlane (and covers M0 -> DMA).
__device__ __forceinline__ void glds16_so(const void* sbase, unsigned voff, void* lds_base) {
  const unsigned lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)LDS_PTR(void, lds_base));
  TRIAD_LDS_DMA_CHECK(lds, 1);
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 2\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds)
      : "memory");
}

// The same with the destination as an LDS byte address in a scalar register (the multi-tile kernel:
// `ptr + elements` of a bf16 image pointer written for addresses, so the staging code below serves
// both). The multi-tile loop makes the base opaque once per k-step, so a piece's address is one
// scalar add in the loop and not one of 32 loop-invariant registers the loop has no room for.
struct GtLds {
  unsigned addr;
  __device__ __forceinline__ GtLds operator+(int elems) const { return GtLds{addr + 2u * (unsigned)elems}; }
};

__device__ __forceinline__ void glds16_so(const void* sbase, unsigned voff, GtLds dst) {
  TRIAD_LDS_DMA_CHECK(dst.addr, 2);
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 2\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(dst.addr)
      : "memory");
}

// per-lane byte offset of a piece of parity j: row lane >> 3 (k-row lane >> 4) and the swizzled chunk
template <bool KCONTIG>
__device__ __forceinline__ unsigned gp_voff(long long ld, int lane, int j) {
  if (KCONTIG) {
    const int mr = lane >> 3, c = (lane & 7) ^ (((j * 8 + mr) >> 1) & 7);
    return (unsigned)((mr * ld + c * 8) * 2);
  }
  const int kr = lane >> 4, c = (lane & 15) ^ ((kr & 3) << 2);
  return (unsigned)((kr * ld + c * 8) * 2);
}

template <bool KCONTIG, typename D>
__device__ __forceinline__ void gp_piece(const bf16* __restrict__ X, long long ld, int r0, int k0, D img, int inst,
                                         unsigned voff) {
  if (KCONTIG) {
    glds16_so(X + (size_t)(r0 + inst * 8) * ld + k0, voff, img + inst * 512);
  } else {
    const int half = inst >> 4, ii = inst & 15;
    glds16_so(X + (size_t)(k0 + ii * 4) * ld + r0 + half * 128, voff, img + half * (BK * 128) + ii * 512);
  }
}

template <bool KCONTIG, bool SUBS, typename D>
__device__ __forceinline__ void gp_half(const bf16* __restrict__ X, long long ld, int r0, int k0, D img, int wave,
                                        const unsigned (&voff)[2], int hh) {
#pragma unroll
  for (int j = 0; j < GP_LOADS; ++j) {
    const int k = wave * 2 + j;
    const int inst = SUBS ? (k >> 2) * 8 + hh * 4 + (k & 3) : wave * 4 + hh * 2 + j;   // inst & 1 == j
    gp_piece<KCONTIG>(X, ld, r0, k0, img, inst, voff[j]);
  }
}

// end of a phase's read / issue part: this wave's fragment reads retired, then the barrier
__device__ __forceinline__ void gp_sync() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// the 8 MFMAs of quadrant (rows 64 ah .. + 63, cols 32 b .. + 31) over the four 16-deep steps
__device__ __forceinline__ void gp_quadrant(f32x16 (&acc)[4][2], const bf16x8 (&af)[2][4], const bf16x8 (&bf)[4], int ah,
                                            int b, bool trail = true) {
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int s = 0; s < BK / 16; ++s)
#pragma unroll
    for (int a = 0; a < 2; ++a) acc[2 * ah + a][b] = mfma32(af[a][s], bf[s], acc[2 * ah + a][b]);
  __builtin_amdgcn_s_setprio(0);
  __builtin_amdgcn_sched_barrier(0);
  if (trail) __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

struct GpNoHook {};   // gp_step's p3_scalar of the one-tile kernel: nothing

// The k-step of one stage from slot `slot` (a constant in the loop). A1 at (m1, k1) = the A rows
// and k offset of the next stage, A2 / B2 at (m2, n2, k2) = the tile origin and k offset of the
// stage after that: the one-tile kernel passes its operands and its own tile at kn and kn + BK,
// the multi-tile kernel pointers to whatever tile those stages belong to (and zeros). dst = the
// two slots as the LDS-DMA's destination: lds itself, or its address (GtLds).
template <bool A_KCONTIG, bool B_KCONTIG, int MODE, typename D, typename H>
__device__ __forceinline__ void gp_step(const bf16* __restrict__ A1, const bf16* __restrict__ A2, long long lda,
                                        const bf16* __restrict__ B2, long long ldb, int m1, int k1, int m2, int n2,
                                        int k2, bf16* lds, D dst, int slot, int wave, int lane, int wm, int wn,
                                        const unsigned (&va)[2], const unsigned (&vb)[2], f32x16 (&acc)[4][2],
                                        H p3_scalar) {
  const D cur = dst + slot * GW_ST;
  const D oth = dst + (slot ^ 1) * GW_ST;
  const bf16* ai = lds + slot * GW_ST;
  const bf16* bi = ai + GW_A;
  bf16x8 af[2][4], bfr[2][4];
  // p0
#pragma unroll
  for (int s = 0; s < 4; ++s) bfr[0][s] = gw_frag<B_KCONTIG>(bi, wn * 64, s, lane);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int s = 0; s < 4; ++s) af[a][s] = gw_frag<A_KCONTIG>(ai, wm * 128 + a * 32, s, lane);
  if (!B_KCONTIG)
#pragma unroll
    for (int s = 0; s < 4; ++s) bfr[1][s] = gw_frag<B_KCONTIG>(bi, wn * 64 + 32, s, lane);
  __builtin_amdgcn_sched_barrier(0);
  if (MODE != GP_LAST) gp_half<A_KCONTIG, false>(A1, lda, m1, k1, oth, wave, va, 1);
  gp_sync();
  gp_quadrant(acc, af, bfr[0], 0, 0);
  // p1
  if (B_KCONTIG)
#pragma unroll
    for (int s = 0; s < 4; ++s) bfr[1][s] = gw_frag<B_KCONTIG>(bi, wn * 64 + 32, s, lane);
  __builtin_amdgcn_sched_barrier(0);
  if (MODE == GP_STEADY) gp_half<B_KCONTIG, B_KCONTIG>(B2, ldb, n2, k2, cur + GW_A, wave, vb, 0);
  gp_sync();
  gp_quadrant(acc, af, bfr[1], 0, 1);
  // p2
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int s = 0; s < 4; ++s) af[a][s] = gw_frag<A_KCONTIG>(ai, wm * 128 + 64 + a * 32, s, lane);
  __builtin_amdgcn_sched_barrier(0);
  if (MODE == GP_STEADY) gp_half<B_KCONTIG, B_KCONTIG>(B2, ldb, n2, k2, cur + GW_A, wave, vb, 1);
  gp_sync();
  gp_quadrant(acc, af, bfr[1], 1, 1);
  // p3 (the phase with no fragment reads: the multi-tile kernel's scalar bookkeeping rides here)
  if constexpr (!std::is_same<H, GpNoHook>::value) p3_scalar();
  if (MODE == GP_STEADY) {
    gp_half<A_KCONTIG, false>(A2, lda, m2, k2, cur, wave, va, 0);
    TRIAD_VMCNT(GP_LOADS * GP_FLIGHT);
  } else if (MODE == GP_PENULT) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  gp_sync();
  // the last barrier of the last k-step: only wm = 0 executes it (it is wm = 1's barrier before
  // these MFMAs), which evens out the one barrier wm = 1 ran more at the start
  gp_quadrant(acc, af, bfr[0], 1, 0, MODE != GP_LAST || wm == 0);
}

template <bool A_KCONTIG, bool B_KCONTIG, typename OutT>
__global__ __launch_bounds__(512, 1) void gemm_w8_kernel(const bf16* __restrict__ A, long long lda,
                                                         const bf16* __restrict__ B, long long ldb, int M, int N,
                                                         int Kd, const float* __restrict__ alpha_p,
                                                         OutT* __restrict__ C, long long ldc, int k_per_split,
                                                         long long slab_stride, const void* __restrict__ bias, int bias_bf16, int xsplit) {
  __shared__ __attribute__((aligned(16))) bf16 lds[2 * GW_ST];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int h = lane >> 5;
  int swz, split;
  tile_split(xsplit, swz, split);
  const int ntn = N / GW_N;
  const int m0 = (swz / ntn) * GW_M, n0 = (swz % ntn) * GW_N;

  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f32x16){};

  const int kbeg = split * k_per_split;
  const int nk = __builtin_amdgcn_readfirstlane(max(0, min(k_per_split, Kd - kbeg)) / BK);
  C += (size_t)split * slab_stride;
  if (nk > 0) {
    const unsigned va[2] = {gp_voff<A_KCONTIG>(lda, lane, 0), gp_voff<A_KCONTIG>(lda, lane, 1)};
    const unsigned vb[2] = {gp_voff<B_KCONTIG>(ldb, lane, 0), gp_voff<B_KCONTIG>(ldb, lane, 1)};
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      gp_half<B_KCONTIG, B_KCONTIG>(B, ldb, n0, kbeg, lds + GW_A, wave, vb, hh);
      gp_half<A_KCONTIG, false>(A, lda, m0, kbeg, lds, wave, va, hh);
    }
    if (nk > 1) {
      gp_half<B_KCONTIG, B_KCONTIG>(B, ldb, n0, kbeg + BK, lds + GW_ST + GW_A, wave, vb, 0);
      gp_half<B_KCONTIG, B_KCONTIG>(B, ldb, n0, kbeg + BK, lds + GW_ST + GW_A, wave, vb, 1);
      gp_half<A_KCONTIG, false>(A, lda, m0, kbeg + BK, lds + GW_ST, wave, va, 0);
      TRIAD_VMCNT(GP_LOADS * GP_FLIGHT);
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    if (wm) __builtin_amdgcn_s_barrier();   // the stagger
    __builtin_amdgcn_sched_barrier(0);
#define GP_STEP(slot, MODE, kt)                                                                                \
  gp_step<A_KCONTIG, B_KCONTIG, MODE>(A, A, lda, B, ldb, m0, kbeg + ((kt) + 1) * BK, m0, n0, kbeg + ((kt) + 2) * BK, \
                                      lds, lds, slot, wave, lane, wm, wn, va, vb, acc, GpNoHook{})
    int kt = 0;
    for (; kt + 3 < nk; kt += 2) {
      GP_STEP(0, GP_STEADY, kt);
      GP_STEP(1, GP_STEADY, kt + 1);
    }
    // 1 (nk = 1 only), 2 or 3 k-steps are left and kt is even
    if (nk - kt == 3) {
      GP_STEP(0, GP_STEADY, kt);
      ++kt;
    }
    if (nk - kt == 2) {
      GP_STEP(kt & 1, GP_PENULT, kt);
      ++kt;
    }
    GP_STEP(kt & 1, GP_LAST, kt);
#undef GP_STEP
  }

  const float alpha = alpha_p ? *alpha_p : 1.f;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int n = n0 + wn * 64 + b * 32 + (lane & 31);
      const float bn = bias_at(bias, bias_bf16, n);
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int m = m0 + wm * 128 + a * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
        C[(size_t)m * ldc + n] = (OutT)(alpha * acc[a][b][v] + bn);
      }
    }
}

// ---- the multi-tile form: one workgroup runs several 256 x 256 tiles back to back ----------------
// Workgroup g of W = gridDim.x takes the tiles of linear index g, g + W, g + 2 W, ... (< tiles),
// each mapped through tile_split's XCD remap with T = tiles, and runs the pipelined loop above over
// the CONCATENATION of their k loops: number the workgroup's stages s = 0, 1, ... across all its
// tiles, stage s = k-step s % nk of its (s / nk)-th tile, living in slot s & 1. The issue schedule
// is the one-tile kernel's with kt read as s (p0: A half 1 of stage s + 1; p1-p3: B half 0, B half
// 1, A half 0 of stage s + 2; vmcnt(GP_LOADS * GP_FLIGHT) in p3); only the source addresses differ:
// the (m0, n0, k) of stages s + 1 and s + 2 are carried in scalar registers (GtCur) and may belong
// to the next tile, or with nk = 1 to the tile after that. The RAW / WAR argument above speaks only
// of stages, slots and phases, so it holds for the flattened sequence as written: p3's wait of
// stage s retires all of stage s + 1 before any wave reads it in phase 4 (s + 1), and every slot
// half is restaged one phase after its last read, whichever tile the new data belongs to. The DMA
// never drains between tiles; the prologue runs once per workgroup and GP_PENULT / GP_LAST are the
// workgroup's last two stages overall.
// The seam: after the trailing barrier of the p3 MFMA cluster of a tile's last k-step, behind a
// scalar branch, each wave writes that tile out (alpha, bias, cast, 128 stores) and zeroes its
// accumulators. The seam has no barrier, so every wave still executes 8 barriers per stage and
// 1 + 8 x (total stages) in all (wm = 0: 1 + 8 S; wm = 1: 1 + 1 for the stagger + 8 S - 1, the
// trailing barrier of the workgroup's last stage), set up and evened out once per workgroup. While
// wm = 0 writes, wm = 1 runs its p3 cluster; while wm = 1 writes, wm = 0 runs the next tile's p0.
// The k order per accumulator and the epilogue arithmetic are the one-tile kernel's: outputs are
// bit-equal.
// vmcnt at the seam: stores count in vmcnt too and may retire out of order with loads, so the next
// p3 wait may also wait for stores. It cannot wait for too little: LDS-DMA loads retire in order
// among themselves, and after vmcnt(6) at most 6 operations of any kind are outstanding, hence at
// most the 6 youngest loads -- the stage the wait is for has landed. (The counter has 6 bits: a
// wave with 63 operations outstanding stalls at issue, so the 128 stores throttle themselves.)
// Bias: an ordinary load in the seam would make hipcc drain the DMA with vmcnt(0), so each wave
// stages its own 64 bias values by one 4-byte-per-lane LDS-DMA (a bf16 bias by the 2-byte form,
// zero-extended) into its 256 bytes of one of two regions behind the slots (the same __shared__
// array), the region of tile ordinal j being j & 1. It is issued ahead of p0 of the stage BEFORE
// the tile's first (the first tile's in the prologue), so that stage's p3 wait retires it (it is
// older than the three half-tiles the wait leaves in flight) at least a whole k-step and eight
// barriers before the seam reads it; the region's previous reader is the seam of tile j - 2, which
// the issuing wave -- the only wave that reads or writes these 256 bytes -- has left by then.
constexpr int GT_BIAS = 8 * 64 * 2;   // bf16 elements of one bias region: 8 waves x 64 dwords

// 64 consecutive bias values -> 64 LDS dwords at lds_base (wave-uniform), lane l value l. The
// per-lane offset is made inside the statement (v_mbcnt), not carried through the loop in a VGPR
// the loop has no room for.
__device__ __forceinline__ void gt_bias_dma(const void* bias, int bias_bf16, int n, void* lds_base) {
  const unsigned lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)LDS_PTR(void, lds_base));
  unsigned keep, voff;
  if (bias_bf16)
    asm volatile(
        "v_mbcnt_lo_u32_b32 %1, -1, 0\n\t"
        "v_mbcnt_hi_u32_b32 %1, -1, %1\n\t"
        "v_lshlrev_b32 %1, 1, %1\n\t"
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 2\n\t"
        "global_load_lds_ushort %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep), "=&v"(voff)
        : "s"((const bf16*)bias + n), "s"(lds)
        : "memory");
  else
    asm volatile(
        "v_mbcnt_lo_u32_b32 %1, -1, 0\n\t"
        "v_mbcnt_hi_u32_b32 %1, -1, %1\n\t"
        "v_lshlrev_b32 %1, 2, %1\n\t"
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 2\n\t"
        "global_load_lds_dword %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep), "=&v"(voff)
        : "s"((const bf16*)bias + 2 * n), "s"(lds)
        : "memory");
}

// a stage of a workgroup's flattened sequence: tile origin, k offset, ordinal of the tile
// and its operands at (m0, k) / (n0, k): a piece's source is pa / pb + a per-wave constant
struct GtCur {
  int m0, n0, k, j;
  const bf16* pa;
  const bf16* pb;
};

template <bool A_KCONTIG, bool B_KCONTIG>
__device__ __forceinline__ void gt_origin(GtCur& c, const bf16* A, long long lda, const bf16* B, long long ldb,
                                          int tiles, int ntn) {
  // past the workgroup's last tile the origin is never used (GP_PENULT / GP_LAST issue no such load)
  const int t = xcd_tile((int)blockIdx.x + c.j * (int)gridDim.x, tiles);
  c.m0 = (t / ntn) * GW_M;
  c.n0 = (t % ntn) * GW_N;
  c.pa = A + (A_KCONTIG ? (size_t)c.m0 * lda : (size_t)c.m0);
  c.pb = B + (B_KCONTIG ? (size_t)c.n0 * ldb : (size_t)c.n0);
}

template <bool A_KCONTIG, bool B_KCONTIG>
__device__ __forceinline__ GtCur gt_next(GtCur c, const bf16* A, long long lda, const bf16* B, long long ldb, int Kd,
                                         int tiles, int ntn) {
  c.k += BK;
  if (c.k == Kd) {
    c.k = 0;
    ++c.j;
    gt_origin<A_KCONTIG, B_KCONTIG>(c, A, lda, B, ldb, tiles, ntn);
  } else {
    c.pa += A_KCONTIG ? (long long)BK : BK * lda;
    c.pb += B_KCONTIG ? (long long)BK : BK * ldb;
  }
  return c;
}

// One output element to row base `row` (scalar registers) + voff (per lane) + OFF bytes. An asm store
// pins the scalar-base form: written in C++, hipcc folds base + voff into 128 per-lane 64-bit
// pointers and their row arithmetic into the seam (measured: ~800 scalar and ~80 vector instructions
// per seam and wave). hipcc does not count an asm store; nothing in the kernel waits for one.
template <int OFF>
__device__ __forceinline__ void gt_store1(const char* row, unsigned voff, float x) {
  asm volatile("global_store_dword %0, %1, %2 offset:%3" ::"v"(voff), "v"(x), "s"(row), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void gt_store1(const char* row, unsigned voff, bf16 x) {
  asm volatile("global_store_short %0, %1, %2 offset:%3" ::"v"(voff), "v"(x), "s"(row), "n"(OFF) : "memory");
}

// The one-tile kernel's epilogue arithmetic on tile (m0, n0), the bias from this wave's 64 staged
// dwords, then the accumulators zeroed. Rows are walked with one scalar pointer: a lane's rows are
// 32 a + 8 q + i (+ 4 h in voff), so the next row is always 1 or 5 rows on; the two 32-column
// blocks of a row are the store's immediate offset.
template <typename OutT>
__device__ __forceinline__ void gt_store(f32x16 (&acc)[4][2], OutT* __restrict__ C, long long ldc, int m0, int n0,
                                         float alpha, const unsigned* bl, bool has_bias, int bias_bf16, int wm, int wn,
                                         int lane) {
  const int h = lane >> 5;
  float bn[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const unsigned raw = bl[b * 32 + (lane & 31)];
    bn[b] = has_bias ? __uint_as_float(bias_bf16 ? raw << 16 : raw) : 0.f;
  }
  const unsigned voff = (unsigned)((4 * h * ldc + (lane & 31)) * (long long)sizeof(OutT));
  const long long rs = ldc * (long long)sizeof(OutT);
  const char* row = (const char*)(C + (size_t)(m0 + wm * 128) * ldc + n0 + wn * 64);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      gt_store1<0>(row, voff, (OutT)(alpha * acc[a][0][v] + bn[0]));
      gt_store1<32 * (int)sizeof(OutT)>(row, voff, (OutT)(alpha * acc[a][1][v] + bn[1]));
      row += (v & 3) == 3 ? 5 * rs : rs;
      asm volatile("" : "+s"(row));   // keep the walk a chain of scalar adds
    }
    acc[a][0] = (f32x16){};
    acc[a][1] = (f32x16){};
  }
}

template <bool A_KCONTIG, bool B_KCONTIG, typename OutT>
__global__ __launch_bounds__(512, 1) void gemm_w8_tiles_kernel(const bf16* __restrict__ A, long long lda,
                                                               const bf16* __restrict__ B, long long ldb, int N,
                                                               int Kd, const float* __restrict__ alpha_p,
                                                               OutT* __restrict__ C, long long ldc,
                                                               const void* __restrict__ bias, int bias_bf16,
                                                               int tiles) {
  __shared__ __attribute__((aligned(16))) bf16 lds[2 * GW_ST + 2 * GT_BIAS];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int ntn = N / GW_N;
  const int W = gridDim.x;
  const int cnt = (tiles - (int)blockIdx.x + W - 1) / W;   // this workgroup's tiles, >= 1 (W <= tiles)
  const int S = cnt * (Kd / BK);                            // its stages
  const float alpha = alpha_p ? *alpha_p : 1.f;
  const bool has_bias = bias != nullptr;
  bf16* const bias_lds = lds + 2 * GW_ST + wave * 128;      // + (j & 1) * GT_BIAS

  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f32x16){};

  const unsigned va[2] = {gp_voff<A_KCONTIG>(lda, lane, 0), gp_voff<A_KCONTIG>(lda, lane, 1)};
  const unsigned vb[2] = {gp_voff<B_KCONTIG>(ldb, lane, 0), gp_voff<B_KCONTIG>(ldb, lane, 1)};
#define GT_NEXT(c) gt_next<A_KCONTIG, B_KCONTIG>(c, A, lda, B, ldb, Kd, tiles, ntn)
  GtCur c0 = {0, 0, 0, 0, nullptr, nullptr};
  gt_origin<A_KCONTIG, B_KCONTIG>(c0, A, lda, B, ldb, tiles, ntn);
  GtCur c1 = GT_NEXT(c0), c2 = GT_NEXT(c1);   // stages s + 1, s + 2
  const GtLds dma = {(unsigned)(size_t)LDS_PTR(void, lds)};
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    gp_half<B_KCONTIG, B_KCONTIG>(c0.pb, ldb, 0, 0, dma + GW_A, wave, vb, hh);
    gp_half<A_KCONTIG, false>(c0.pa, lda, 0, 0, dma, wave, va, hh);
  }
  if (has_bias) gt_bias_dma(bias, bias_bf16, c0.n0 + wn * 64, bias_lds);
  if (S > 1) {
    gp_half<B_KCONTIG, B_KCONTIG>(c1.pb, ldb, 0, 0, dma + (GW_ST + GW_A), wave, vb, 0);
    gp_half<B_KCONTIG, B_KCONTIG>(c1.pb, ldb, 0, 0, dma + (GW_ST + GW_A), wave, vb, 1);
    gp_half<A_KCONTIG, false>(c1.pa, lda, 0, 0, dma + GW_ST, wave, va, 0);
    TRIAD_VMCNT(GP_LOADS * GP_FLIGHT);
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  if (wm) __builtin_amdgcn_s_barrier();   // the stagger
  __builtin_amdgcn_sched_barrier(0);
  // One stage: the next tile's bias if stage s + 1 opens a tile (never in GP_LAST: no stage s + 1),
  // the k-step, the seam if it closed a tile. The three cursors move on by one stage in p3, which
  // has no fragment reads to issue (the step took its sources by value); `e` = the stage the
  // k-step was for.
  GtCur e = c0;
  bool bias_next = has_bias && c1.k == 0;
#define GT_STEP(slot, MODE)                                                                                       \
  do {                                                                                                            \
    if (MODE != GP_LAST && bias_next)                                                                             \
      gt_bias_dma(bias, bias_bf16, c1.n0 + wn * 64, bias_lds + (c1.j & 1) * GT_BIAS);                             \
    GtLds dst = dma;                                                                                              \
    asm volatile("" : "+s"(dst.addr));                                                                            \
    gp_step<A_KCONTIG, B_KCONTIG, MODE>(c1.pa, c2.pa, lda, c2.pb, ldb, 0, 0, 0, 0, 0, lds, dst, slot, wave, lane,  \
                                        wm, wn, va, vb, acc, [&] {                                                \
                                          e = c0;                                                                 \
                                          c0 = c1;                                                                \
                                          c1 = c2;                                                                \
                                          c2 = GT_NEXT(c2);                                                       \
                                          bias_next = has_bias && c1.k == 0;                                      \
                                        });                                                                       \
    if (MODE == GP_LAST || e.k + BK == Kd) {                                                                      \
      gt_store<OutT>(acc, C, ldc, e.m0, e.n0, alpha, (const unsigned*)(bias_lds + (e.j & 1) * GT_BIAS), has_bias,  \
                     bias_bf16, wm, wn, lane);                                                                    \
      __builtin_amdgcn_sched_barrier(0);                                                                          \
    }                                                                                                             \
  } while (0)
  int s = 0;
  for (; s + 3 < S; s += 2) {
    GT_STEP(0, GP_STEADY);
    GT_STEP(1, GP_STEADY);
  }
  // 1 (S = 1 only), 2 or 3 stages are left and s is even
  if (S - s == 3) {
    GT_STEP(0, GP_STEADY);
    ++s;
  }
  if (S - s == 2) {
    GT_STEP(s & 1, GP_PENULT);
    ++s;
  }
  GT_STEP(s & 1, GP_LAST);
#undef GT_STEP
#undef GT_NEXT
}

// (Measured and not kept, round 4: the eight-wave tile on v_mfma_f32_16x16x32_bf16 -- bit-identical,
// but 2-30 % slower on every c3 projection-head / backbone shape, profiles/r04_gemm_m16_ab.log; the
// 16 x 16 x 32 shape pays off in the similarity head's direct-B tile GEMMs, not here.)

// The 256 x 256 form the size policy picks for tall outputs: the eight-wave form (4), 3-13 % faster
// than the four-wave form (3) on every c3 backbone / projection-head shape with M >= 50,944
// (profiles/r02_gemm_w8_probe.log). (Measured and not kept: the eight-wave tile on a 4-slot ring of
// 32-deep chunks with the DMA three chunks ahead, 5-8 % slower than this two-slot 64-deep form on
// every M >= 50,944 shape, profiles/r02_gemm_w8_ring_probe.log.) Tile forms are per-call arguments
// (triad_gemm_bf16_form, triad_gemm_bf16_splitk_form): there is no process-wide GEMM state.
constexpr int kBigForm = 4;
// form flag of the split-K entry points: the workgroups of one split all on one XCD (tile_split)
constexpr int kXcdSplit = 8;
// HIP's limit on gridDim.y, where the split index lives
constexpr int kMaxGridY = 65535;


// Grid of the multi-tile kernel for `tiles` output tiles on `cus` CUs, 0 = one tile per workgroup.
// With R = ceil(tiles / cus) dispatch rounds, ceil(tiles / R) workgroups of at most R tiles each:
// the same makespan in tile-times as the dispatcher's rounds (597 tiles on 256 CUs: 199 workgroups
// of 3), and the tiles live at one time stay neighbours. The tail of a fractional round is left as
// it is.
int w8_workgroups(int tiles, int cus) {
  const int R = (tiles + cus - 1) / cus;
  return R <= 1 ? 0 : (tiles + R - 1) / R;
}

// the multi-tile kernel's per-lane store offset (4 rows of C, in bytes) is a 32-bit register
constexpr long long kTilesMaxLdc = 1LL << 27;

// CU count of the current device, read once per device ordinal
int device_cus() {
  constexpr int kDevs = 64;
  static std::atomic<int> cache[kDevs];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  int cus = dev >= 0 && dev < kDevs ? cache[dev].load(std::memory_order_relaxed) : 0;
  if (cus <= 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    if (dev >= 0 && dev < kDevs) cache[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

// tile_wgs: 0 = the product path (a splits == 1 call in the eight-wave form is routed to the
// multi-tile kernel when some workgroup would get a second tile); > 0 = the multi-tile kernel on
// that grid (triad_gemm_bf16_tiles).
template <bool AK, bool BK_, typename OutT>
int launch(const void* A, long long lda, const void* B, long long ldb, int M, int N, int Kd, const float* alpha,
           void* C, long long ldc, hipStream_t st, int splits = 1, long long slab_stride = 0,
           const void* bias = nullptr, int form = 0, int bias_bf16 = 0, int tile_wgs = 0) {
  const int xsplit = (form & kXcdSplit) ? 1 : 0;
  form &= ~kXcdSplit;
  if (M <= 0 || N <= 0 || Kd <= 0) return TRIAD_EINVAL;
  if (M % BM || N % BN || Kd % BK || lda % 8 || ldb % 8 || splits < 1) return TRIAD_EINVAL;
  if (xsplit && splits % 8) return TRIAD_EINVAL;
  if (splits > kMaxGridY) return TRIAD_EINVAL;   // blockIdx.y is the split
  if (!A || !B || !C || ldc < N) return TRIAD_EINVAL;
  // every operand piece is a 16-byte LDS-DMA (glds16): with lda, ldb % 8 == 0 above, aligned bases
  // make every piece aligned. (No lda >= Kd rule: the conv stack's A rows overlap, lda < Kd.)
  if ((uintptr_t)A % 16 || (uintptr_t)B % 16) return TRIAD_EINVAL;
  const int kps = ((Kd / BK + splits - 1) / splits) * BK;
  // the 256-row ring pays off on long k loops or many row tiles (conv / projection GEMMs);
  // the short split-K weight-gradient loops keep the 128 x 128 form (measured, profiles/r01_dw_gemm_*.log)
  const bool w4_ok = M % GW_M == 0 && N % GW_N == 0;
  // the four-wave form measured faster on the long conv-stack GEMMs (tools/gemm_forms.py:
  // 2.94 -> 2.67 ms at M = 1.6 M, N = 512, K = 1536); the split-K weight gradients and the
  // shorter forward shapes keep the smaller tiles
  const bool w4_auto = AK && BK_ && splits == 1 && M >= 65536 && Kd >= 1024;
  if (tile_wgs) {
    if (!w4_ok || splits != 1 || tile_wgs < 1 || tile_wgs > (long long)(M / GW_M) * (N / GW_N)) return TRIAD_EINVAL;
    if (ldc > kTilesMaxLdc) return TRIAD_EINVAL;
    form = kBigForm;
  }
  if (form == 0 && w4_ok && w4_auto) form = kBigForm;
  if (w4_ok && (form == 4 || form == 3)) {   // (form 3, the four-wave 256 x 256 tile, was retired in round 5)
    const int nwg = (M / GW_M) * (N / GW_N);
    if (!tile_wgs && splits == 1 && ldc <= kTilesMaxLdc) tile_wgs = w8_workgroups(nwg, device_cus());
    if (tile_wgs) {
      hipLaunchKernelGGL((gemm_w8_tiles_kernel<AK, BK_, OutT>), dim3(tile_wgs), dim3(512), 0, st, (const bf16*)A, lda,
                         (const bf16*)B, ldb, N, Kd, alpha, (OutT*)C, ldc, bias, bias_bf16, nwg);
      TRIAD_CHECK_LAUNCH();
      return TRIAD_OK;
    }
    hipLaunchKernelGGL((gemm_w8_kernel<AK, BK_, OutT>), dim3(nwg, splits), dim3(512), 0, st, (const bf16*)A, lda,
                       (const bf16*)B, ldb, M, N, Kd, alpha, (OutT*)C, ldc, kps, slab_stride, bias, bias_bf16, xsplit);
    TRIAD_CHECK_LAUNCH();
    return TRIAD_OK;
  }
  if (form != 1 && M % GB_M == 0 &&
      (form == 2 || M >= 8192 || Kd / splits >= 32768)) {
    const int nwg = (M / GB_M) * (N / BN);
    hipLaunchKernelGGL((gemm_big_kernel<AK, BK_, OutT>), dim3(nwg, splits), dim3(512), 0, st, (const bf16*)A, lda,
                       (const bf16*)B, ldb, M, N, Kd, alpha, (OutT*)C, ldc, kps, slab_stride, bias, bias_bf16, xsplit);
    TRIAD_CHECK_LAUNCH();
    return TRIAD_OK;
  }
  const int nwg = (M / BM) * (N / BN);
  hipLaunchKernelGGL((gemm_kernel<AK, BK_, OutT>), dim3(nwg, splits), dim3(256), 0, st, (const bf16*)A, lda,
                     (const bf16*)B, ldb, M, N, Kd, alpha, (OutT*)C, ldc, kps, slab_stride, bias, bias_bf16, xsplit);
  TRIAD_CHECK_LAUNCH();
  return TRIAD_OK;
}

}  // namespace

extern "C" {

// C[M][N] = alpha * op(A) . op(B). a_kcontig=1: A stored [M][Kd] (lda), 0: [Kd][M].
// b_kcontig=1: B stored [N][Kd] (ldb), 0: [Kd][N]. out_bf16 selects a bf16 or fp32 C.
// form: 0 = the size policy of launch(), 1 = 128 x 128, 2 = 256 x 128 ring, 3 = (retired four-wave, runs as 4),
// 4 = 256 x 256 eight-wave (3 / 4 when M, N are multiples of 256; otherwise the policy's fallback).
int triad_gemm_bf16_form(const void* A, long long lda, int a_kcontig, const void* B, long long ldb, int b_kcontig,
                         int M, int N, int Kd, const float* alpha, void* C, long long ldc, int out_bf16, int form,
                         hipStream_t stream) {
  if (form < 0 || form > 4) return TRIAD_EINVAL;
#define TRIAD_GEMM_CASE(AK, BKC)                                                                  \
  if (!!a_kcontig == AK && !!b_kcontig == BKC)                                                   \
    return out_bf16 ? launch<AK, BKC, bf16>(A, lda, B, ldb, M, N, Kd, alpha, C, ldc, stream, 1, 0, nullptr, form) \
                    : launch<AK, BKC, float>(A, lda, B, ldb, M, N, Kd, alpha, C, ldc, stream, 1, 0, nullptr, form);
  TRIAD_GEMM_CASE(true, true)
  TRIAD_GEMM_CASE(true, false)
  TRIAD_GEMM_CASE(false, true)
  TRIAD_GEMM_CASE(false, false)
#undef TRIAD_GEMM_CASE
  return TRIAD_EINVAL;
}

// Grid the 256 x 256 eight-wave form runs `tiles` output tiles on, on a device of `cus` CUs: the
// workgroup count of the multi-tile kernel, or 0 when every workgroup gets one tile (the one-tile
// kernel). Host only.
int triad_gemm_w8_workgroups(int tiles, int cus) {
  if (tiles <= 0 || cus <= 0) return TRIAD_EINVAL;
  return w8_workgroups(tiles, cus);
}

// The multi-tile eight-wave kernel on a caller-chosen grid, 1 <= workgroups <= (M / 256)(N / 256):
// workgroup g runs tiles g, g + workgroups, ... back to back. M, N multiples of 256. For tests and
// tools; the product entry points route themselves (launch()).
int triad_gemm_bf16_tiles(const void* A, long long lda, int a_kcontig, const void* B, long long ldb, int b_kcontig,
                          int M, int N, int Kd, const float* alpha, void* C, long long ldc, int out_bf16,
                          const void* bias, int bias_bf16, int workgroups, hipStream_t stream) {
  if (workgroups < 1) return TRIAD_EINVAL;
#define TRIAD_GEMM_T(AK, BKC)                                                                                 \
  if (!!a_kcontig == AK && !!b_kcontig == BKC)                                                                \
    return out_bf16 ? launch<AK, BKC, bf16>(A, lda, B, ldb, M, N, Kd, alpha, C, ldc, stream, 1, 0, bias, 0,    \
                                            !!bias_bf16, workgroups)                                          \
                    : launch<AK, BKC, float>(A, lda, B, ldb, M, N, Kd, alpha, C, ldc, stream, 1, 0, bias, 0,   \
                                             !!bias_bf16, workgroups);
  TRIAD_GEMM_T(true, true)
  TRIAD_GEMM_T(true, false)
  TRIAD_GEMM_T(false, true)
  TRIAD_GEMM_T(false, false)
#undef TRIAD_GEMM_T
  return TRIAD_EINVAL;
}

int triad_gemm_bf16(const void* A, long long lda, int a_kcontig, const void* B, long long ldb, int b_kcontig,
                    int M, int N, int Kd, const float* alpha, void* C, long long ldc, int out_bf16,
                    hipStream_t stream) {
  return triad_gemm_bf16_form(A, lda, a_kcontig, B, ldb, b_kcontig, M, N, Kd, alpha, C, ldc, out_bf16, 0, stream);
}

// The backbone projections (torch's F.linear / matmul under autocast, routed here by
// triad_amd/gemm.py): C = op(A) op(B) (+ bias[n] before the one bf16 rounding), bf16 out. Tile
// form by shape, measured on the c3 shapes (tools/gemm_backend_probe.py,
// profiles/r02_gemm_backend_probe.log, r02_gemm_w8_probe.log): the 256 x 256 eight-wave form when
// the output is tall (M >= 32768, M and N multiples of 256), the 256 x 128 ring for other tall
// outputs, 128 x 128 below 8192 rows. 790-940 TFLOP/s; rocBLAS's own kernels run the same shapes
// at 300-790.
static int gemm_bias_launch(const void* A, long long lda, int a_kcontig, const void* B, long long ldb, int b_kcontig, int M,
                     int N, int Kd, const void* bias, int bias_bf16, void* C, long long ldc, hipStream_t stream) {
  // eight-wave 256 x 256 for every tall output it tiles; the 256 x 128 ring only when its tiles
  // fill the 256 CUs once (the 8,192-row text projection head at N = 512 has 128 such tiles, half
  // the chip, and runs on 256 128 x 128 tiles instead)
  int form = 1;
  if (M >= 32768 && M % GW_M == 0 && N % GW_N == 0) form = kBigForm;
  else if (M >= 8192 && M % GB_M == 0 && (long long)(M / GB_M) * (N / BN) >= 256) form = 2;
#define TRIAD_GEMM_B(AK, BKC)                                                                     \
  if (!!a_kcontig == AK && !!b_kcontig == BKC)                                                    \
    return launch<AK, BKC, bf16>(A, lda, B, ldb, M, N, Kd, nullptr, C, ldc, stream, 1, 0, bias, form, bias_bf16);
  TRIAD_GEMM_B(true, true)
  TRIAD_GEMM_B(true, false)
  TRIAD_GEMM_B(false, true)
  TRIAD_GEMM_B(false, false)
#undef TRIAD_GEMM_B
  return TRIAD_EINVAL;
}

int triad_gemm_bf16_bias(const void* A, long long lda, int a_kcontig, const void* B, long long ldb, int b_kcontig,
                         int M, int N, int Kd, const float* bias, void* C, long long ldc, hipStream_t stream) {
  return gemm_bias_launch(A, lda, a_kcontig, B, ldb, b_kcontig, M, N, Kd, bias, 0, C, ldc, stream);
}

// The same with the bias as the bf16 vector the autocast model holds (F.linear under autocast
// casts the bias to bf16 and adds it in fp32 before the one rounding): no fp32 copy per call.
int triad_gemm_bf16_bias_bf16(const void* A, long long lda, int a_kcontig, const void* B, long long ldb,
                              int b_kcontig, int M, int N, int Kd, const void* bias, void* C, long long ldc,
                              hipStream_t stream) {
  return gemm_bias_launch(A, lda, a_kcontig, B, ldb, b_kcontig, M, N, Kd, bias, 1, C, ldc, stream);
}

// Split-K form for short-and-wide outputs (weight gradients: M, N = 512 / H, Kd = tokens):
// `splits` partial fp32 slabs in `slabs` ([splits][M][N], caller-owned), then
// C = alpha * sum(slabs) as fp32 or bf16 (ldc == N).
// form: as triad_gemm_bf16_form, + 8 (kXcdSplit) = the workgroups of one split all on one XCD
// (needs splits % 8 == 0).
int triad_gemm_bf16_splitk_form(const void* A, long long lda, int a_kcontig, const void* B, long long ldb,
                                int b_kcontig, int M, int N, int Kd, int splits, const float* alpha, float* slabs,
                                void* C, int out_bf16, int form, hipStream_t stream) {
  if ((form & ~kXcdSplit) < 0 || (form & ~kXcdSplit) > 4) return TRIAD_EINVAL;
  if (!slabs || !C) return TRIAD_EINVAL;   // before the slab launch: nothing runs for a call that cannot finish
  const long long slab = (long long)M * N;
  int rc = TRIAD_EINVAL;
#define TRIAD_GEMM_SK(AK, BKC)                                                                  \
  if (!!a_kcontig == AK && !!b_kcontig == BKC)                                                 \
    rc = launch<AK, BKC, float>(A, lda, B, ldb, M, N, Kd, nullptr, slabs, N, stream, splits, slab, nullptr, form);
  TRIAD_GEMM_SK(true, true)
  TRIAD_GEMM_SK(true, false)
  TRIAD_GEMM_SK(false, true)
  TRIAD_GEMM_SK(false, false)
#undef TRIAD_GEMM_SK
  if (rc) return rc;
  return triad_sum_slabs(slabs, splits, slab, alpha, out_bf16, C, stream);
}

int triad_gemm_bf16_splitk(const void* A, long long lda, int a_kcontig, const void* B, long long ldb, int b_kcontig,
                           int M, int N, int Kd, int splits, const float* alpha, float* slabs, void* C,
                           int out_bf16, hipStream_t stream) {
  return triad_gemm_bf16_splitk_form(A, lda, a_kcontig, B, ldb, b_kcontig, M, N, Kd, splits, alpha, slabs, C,
                                     out_bf16, 0, stream);
}

}  // extern "C"
