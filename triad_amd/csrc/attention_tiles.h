// Tile helpers shared by the attention kernels (attention.hip: N <= 320, whole sequence in LDS;
// attention_long.hip: 321 <= N <= 2048, K / V or Q / dO streamed in chunks): the swizzled LDS rows,
// the row and transposed fragment reads, the accumulator-order packs and stores, and the tensor
// check of the C ABI. See the header comment of attention.hip for the layouts.
#pragma once
#include "common.h"

namespace {

constexpr int HD = 64;            // head dim
constexpr float LOG2E = 1.4426950408889634f;

// bit of accumulator element v (row / column (v & 3) + 8 (v >> 2) + 4 h of a 32-wide tile)
__device__ __forceinline__ bool tile_bit(unsigned w, int v, int h) { return (w >> ((v & 3) + 8 * (v >> 2) + 4 * h)) & 1u; }

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

// One tensor of the ABI: non-null, 16-byte aligned, strides in whole bf16x8 vectors (the kernels read
// and write rows with 16- and 8-byte accesses at base + b sB + n sN + 64 h + 8 c).
inline bool row_ok(const void* p, long long sB, long long sN) { return p && !((uintptr_t)p & 15) && !(sB % 8) && !(sN % 8); }

}  // namespace
