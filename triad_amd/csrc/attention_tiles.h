// What the attention translation units share (attention.hip: N <= 320, whole sequence in LDS;
// attention_long.hip: 321 <= N <= 2048, K / V or Q / dO streamed in chunks; attention_mask.hip: the
// dropout keep words of both). Device side: the swizzled LDS rows, the row and transposed fragment
// reads, the accumulator-order packs and stores. Host side: the kernels' argument struct and the one
// copy of every check and field assignment of the C ABI (attn_fwd_args, attn_bwd_args, attn_mask_ok).
// See the header comment of attention.hip for the layouts.
#pragma once
#include "common.h"

namespace {

constexpr int HD = 64;            // head dim
constexpr float LOG2E = 1.4426950408889634f;

// row / column of accumulator element v in a 32-wide tile (h = lane >> 5), and its bit of a keep word
__device__ __forceinline__ int acc_row(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }
__device__ __forceinline__ bool tile_bit(unsigned w, int v, int h) { return (w >> acc_row(v, h)) & 1u; }

__device__ __forceinline__ int swz(int row) {
  const int k = (row >> 1) & 7;
  return (k >> 1) | ((k & 1) << 2);
}
// byte offset of (row, dim d) in a swizzled [rows][64] bf16 LDS array
__device__ __forceinline__ int lds_off(int row, int d) { return row * 128 + (((d >> 3) ^ swz(row)) << 4) + ((d & 7) << 1); }

__device__ __forceinline__ bf16x8 lds_b128(const char* lds, int row, int chunk) {
  return *(const bf16x8*)(lds + row * 128 + ((chunk ^ swz(row)) << 4));
}

// Transposed fragment: lane l of each 16-lane group receives column (colbase + (l & 15)) of rows
// rowbase .. rowbase + 3 (the lane supplies row rowbase + ((l & 15) >> 2), columns 4 (l & 3) ..).
__device__ __forceinline__ s16x4 lds_tr(const char* lds, int rowbase, int colbase, int lane) {
  const int g = lane & 15;
  return lds_tr16(lds + lds_off(rowbase + (g >> 2), colbase + 4 * (g & 3)));
}

// A/B fragment for k = 16 permuted keys (rows) of chunk c: {rows 16c+4h .. +3, 16c+4h+8 .. +11}, column
// colbase + (lane & 15) (+16 for lanes 16-31 of each half)
__device__ __forceinline__ bf16x8 frag_tr(const char* lds, int c, int dimbase, int lane) {
  const int h = lane >> 5;
  const int col = dimbase + 16 * ((lane >> 4) & 1);
  const s16x4 lo = lds_tr(lds, 16 * c + 4 * h, col, lane);
  const s16x4 hi = lds_tr(lds, 16 * c + 4 * h + 8, col, lane);
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

__device__ __forceinline__ bf16x8 pack8(const f32x16& a, int half) {
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = (bf16)a[8 * half + i];
  return r;
}

// 16 values of accumulator element order (row (v&3) + 8(v>>2) + 4h) written as 4 runs of 4
__device__ __forceinline__ void store_cols(bf16* dst, const f32x16& a, float mul, int h) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16x4 w;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (bf16)(a[4 * j + i] * mul);
    *(bf16x4*)(dst + 8 * j + 4 * h) = w;
  }
}

// ---- host side: the argument struct and the C ABI's checks, written once for both families -----------

constexpr int MAX_N_SHORT = 320;   // whole-sequence kernels (attention.hip): 1 .. 320 tokens
constexpr int MAX_N_LONG = 2048;   // streaming kernels (attention_long.hip): 321 .. 2048

struct AttnArgs {
  const bf16 *q, *k, *v, *o, *dout;
  long long q_sB, q_sN, k_sB, k_sN, v_sB, v_sN, o_sB, o_sN, do_sB, do_sN;
  bf16 *out, *dq, *dk, *dv;
  long long out_sB, out_sN, dq_sB, dq_sN, dk_sB, dk_sN, dv_sB, dv_sN;
  float* lse;       // [B*H][N] natural-log log-sum-exp of the scaled scores
  float* delta;     // [B*H][N] rowsum(dO * O)
  int B, H, N;
  float scale;
  // dropout on the attention probabilities (DROP kernels): keep bits by query row
  // wq[(bh * N + q) * wpr + kt] (bit j = key 32 kt + j) and by key row wk[(bh * N + key) * wpr + qt]
  // (bit j = query 32 qt + j); kept probabilities scaled by drop_scale = 1 / (1 - p)
  const unsigned *wq, *wk;
  int wpr;          // words per mask row (attn_wpr)
  float drop_scale;
  // key-padding mask of the whole-sequence kernels (MASK instances; nullptr = none): km[b * wpr + kt], one
  // row of ceil(N / 32) words per SAMPLE (all heads share it), bit j = key 32 kt + j takes part; bits of
  // keys >= N are ignored. Last, so that the fields above keep their kernarg offsets.
  const unsigned* km;
};

// The two kernel families as the checks see them: the token range, and whether a lane reads the two
// keep words of a 64-row chunk as one 8-byte load (rows padded to whole chunks, 8-byte aligned masks).
struct AttnFamily {
  int nmin, nmax;
  bool word_pairs;
};
constexpr AttnFamily ATTN_SHORT = {1, MAX_N_SHORT, false}, ATTN_LONG = {MAX_N_SHORT + 1, MAX_N_LONG, true};

inline int attn_wpr(const AttnFamily& f, int N) { return f.word_pairs ? 2 * ((N + 63) / 64) : (N + 31) / 32; }
// query (dq, forward) or key (dkv) tiles of 32, four per workgroup; blockIdx.y = (sample, head)
inline dim3 attn_grid(int B, int H, int N) { return dim3(((N + 31) / 32 + 3) / 4, B * H); }

// One tensor of the ABI: non-null, 16-byte aligned, strides in whole bf16x8 vectors (the kernels read
// and write rows with 16- and 8-byte accesses at base + b sB + n sN + 64 h + 8 c).
struct AttnRows {
  const void* p;
  long long sB, sN;
};
template <class P>
inline bool attn_rows(const AttnRows& r, P& p, long long& sB, long long& sN) {
  p = (P)r.p; sB = r.sB; sN = r.sN;
  return r.p && !((uintptr_t)r.p & 15) && !(r.sB % 8) && !(r.sN % 8);
}

// Sizes and mask pointers of every entry point: blockIdx.y is the (sample, head) index (<= 65535);
// p in [0, 1) (the comparisons are false for NaN, which triad_drop_thr must never see).
inline bool attn_mask_ok(const AttnFamily& f, int B, int H, int N, float p, const unsigned* wq, const unsigned* wk) {
  const bool aligned = !f.word_pairs || !(((uintptr_t)wq | (uintptr_t)wk) & 7);
  return B > 0 && H > 0 && N >= f.nmin && N <= f.nmax && (long long)B * H <= 65535 && p >= 0.f && p < 1.f && aligned;
}

// Checks and fields the forward and the backward share. The forward takes the row max of the unscaled
// scores (a scale <= 0 would turn it into the row min), so the scale is finite and > 0 (false for NaN).
inline bool attn_qkv_args(AttnArgs& a, const AttnFamily& f, AttnRows q, AttnRows k, AttnRows v, int B, int H, int N,
                          int D, float scale, const unsigned* wq, const unsigned* wk, float p, const float* lse) {
  if (!attn_mask_ok(f, B, H, N, p, wq, wk) || D != HD || !(scale > 0.f && scale < INFINITY) || !lse) return false;
  a.lse = (float*)lse; a.B = B; a.H = H; a.N = N; a.scale = scale;
  a.wq = wq; a.wk = wk; a.wpr = attn_wpr(f, N); a.drop_scale = 1.f / (1.f - p);
  return attn_rows(q, a.q, a.q_sB, a.q_sN) && attn_rows(k, a.k, a.k_sB, a.k_sN) && attn_rows(v, a.v, a.v_sB, a.v_sN);
}

// Validate a forward / backward call of family f and fill the kernels' arguments; false = TRIAD_EINVAL
// (a is then partly written and must not be launched).
inline bool attn_fwd_args(AttnArgs& a, const AttnFamily& f, AttnRows q, AttnRows k, AttnRows v, int B, int H, int N,
                          int D, float scale, const unsigned* wq, float p, AttnRows out, float* lse) {
  return attn_qkv_args(a, f, q, k, v, B, H, N, D, scale, wq, nullptr, p, lse) &&
         attn_rows(out, a.out, a.out_sB, a.out_sN);
}

inline bool attn_bwd_args(AttnArgs& a, const AttnFamily& f, AttnRows q, AttnRows k, AttnRows v, AttnRows o,
                          AttnRows dout, const float* lse, int B, int H, int N, int D, float scale,
                          const unsigned* wq, const unsigned* wk, float p, AttnRows dq, AttnRows dk, AttnRows dv,
                          float* delta) {
  a.delta = delta;
  return attn_qkv_args(a, f, q, k, v, B, H, N, D, scale, wq, wk, p, lse) && (!wq == !wk) && delta &&
         attn_rows(o, a.o, a.o_sB, a.o_sN) && attn_rows(dout, a.dout, a.do_sB, a.do_sN) &&
         attn_rows(dq, a.dq, a.dq_sB, a.dq_sN) && attn_rows(dk, a.dk, a.dk_sB, a.dk_sN) &&
         attn_rows(dv, a.dv, a.dv_sB, a.dv_sN);
}

}  // namespace
