// Keep words of the attention-probability dropout for both attention families (AttnArgs::wq / wk in
// attention_tiles.h): bit of (bh, q, key) = element e = (bh N + q) N + key of the (B H, N, N)
// probability tensor, hashed in pairs by common.h's keep_pair. One kernel writes both layouts with
// wpr words per row: ceil(N / 32) for attention.hip (triad_attn_dropmask), 2 ceil(N / 64) for
// attention_long.hip (triad_attn_long_dropmask: rows padded to whole 64-row chunks).
#include "attention_tiles.h"

namespace {

// Block = the 32-query band qt of one (sample, head), all key tiles: thread (row r, key tile kt)
// hashes its 16 element pairs into the wq word, the band's words meet in LDS and thread (key row j,
// key tile kt) gathers bit j of the 32 words of tile kt into the wk word of key 32 kt + j (query bits
// of tile qt). (One 64-thread block per 32 x 32 tile, 32 threads busy per phase, made this a 90 us
// launch at HuBERT's shape.) nt = ceil(N / 32) tiles; words of tiles that start at or past N
// (wpr > nt: the padding word of an odd tile count) are written as zero in both layouts.
// The LDS array holds the 64 tiles of N = 2048 (8.4 KB) for every call: with 10 tiles (1.3 KB) for
// N <= 320 the kernel's time on MI355X was the same within the spread between two processes.
__global__ __launch_bounds__(256) void attn_dropmask_kernel(int N, int nt, int wpr, unsigned seed, unsigned thr,
                                                            unsigned* __restrict__ wq, unsigned* __restrict__ wk) {
  __shared__ unsigned words[MAX_N_LONG / 32][33];
  const int qt = blockIdx.x;
  const long long bh = blockIdx.y;
  for (int t = threadIdx.x; t < 32 * wpr; t += 256) {
    const int r = t & 31, kt = t >> 5, q = qt * 32 + r;
    unsigned bits = 0u;
    if (q < N) {
      const int ncol = min(32, N - kt * 32);
      if (ncol > 0) {
        const unsigned long long e0 = (unsigned long long)((bh * N + q) * N + kt * 32);
        // pairs covering elements e0 .. e0 + ncol - 1
        const unsigned long long p0 = e0 >> 1;
        const int off = (int)(e0 & 1);
        unsigned long long stream = 0ull;  // bit i = element e0 - off + i
        const int npairs = (ncol + off + 1) >> 1;
#pragma unroll
        for (int i = 0; i < 17; ++i)  // constant shifts (npairs <= 17)
          if (i < npairs) stream |= (unsigned long long)keep_pair(p0 + i, seed, thr) << (2 * i);
        bits = (unsigned)(stream >> off);
        if (ncol < 32) bits &= (1u << ncol) - 1u;
      }
      wq[(bh * N + q) * wpr + kt] = bits;
    }
    if (kt < nt) words[kt][r] = bits;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < 32 * nt; t += 256) {
    const int j = t & 31, kt = t >> 5;  // key row kt * 32 + j: bit i = query qt * 32 + i
    const int key = kt * 32 + j;
    if (key < N) {
      unsigned w = 0u;
#pragma unroll
      for (int i = 0; i < 32; ++i) w |= ((words[kt][i] >> j) & 1u) << i;
      wk[(bh * N + key) * wpr + qt] = w;
      if (qt == nt - 1 && wpr > nt) wk[(bh * N + key) * wpr + nt] = 0u;   // the padding word of an odd tile count
    }
  }
}

int dropmask(const AttnFamily& f, int B, int H, int N, float p, unsigned seed, unsigned* wq, unsigned* wk,
             hipStream_t stream) {
  if (!attn_mask_ok(f, B, H, N, p, wq, wk) || !wq || !wk) return TRIAD_EINVAL;
  const int nt = (N + 31) / 32;
  hipLaunchKernelGGL(attn_dropmask_kernel, dim3(nt, B * H), dim3(256), 0, stream, N, nt, attn_wpr(f, N), seed,
                     triad_drop_thr(p), wq, wk);
  TRIAD_CHECK_LAUNCH();
  return TRIAD_OK;
}

}  // namespace

extern "C" {

int triad_attn_dropmask(int B, int H, int N, float p, unsigned seed, unsigned* wq, unsigned* wk, hipStream_t stream) {
  return dropmask(ATTN_SHORT, B, H, N, p, seed, wq, wk, stream);
}

int triad_attn_long_dropmask(int B, int H, int N, float p, unsigned seed, unsigned* wq, unsigned* wk,
                             hipStream_t stream) {
  return dropmask(ATTN_LONG, B, H, N, p, seed, wq, wk, stream);
}

}  // extern "C"
