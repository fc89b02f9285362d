// Backbone self-attention for short sequences (DINOv2 / HuBERT / DistilBERT under SajayR/TRIAD
// model.py:29-30,79-80,218-227: softmax(Q K^T * scale) V per (sample, head), head dim 64,
// N <= 320 tokens), forward and backward, bf16 in / fp32 accumulate.
//
// A whole (sample, head) sequence fits in LDS, so there is no online softmax: each wave owns a
// 32-token tile and holds all of its scores in registers.
//   forward : wave = query tile; S^T = K Q^T (query on the lane, 10 key tiles max in VGPRs),
//             exact row max / sum (lane-local + one half-wave exchange), O^T = V^T P^T with P^T
//             taken straight from the score registers: the MFMA's k-index is permuted to the
//             keys each lane already holds (k = 8h + i <-> key 16c + 4h + (i & 3) + 8 (i >> 2)),
//             and V^T fragments are transposed LDS reads (ds_read_b64_tr_b16) of row-major V in
//             the same key order. Writes O and the log-sum-exp per query.
//   backward: dq kernel (wave = query tile, same orientation: recompute S, P, dP = dO V^T,
//             dS = P (dP - D), dQ^T += K^T dS^T) and dkv kernel (wave = key tile, key on the
//             lane: S = Q K^T, dP = dO V^T, dV += P^T dO, dK += dS^T Q); D = rowsum(dO * O) is
//             formed by the dq kernel (which reads O anyway) and handed to the dkv kernel.
// Probabilities use the raw v_exp_f32 (__builtin_amdgcn_exp2f; arguments are <= 0 up to rounding,
// results below 2^-126 flush to 0 -- exp2f's denormal scaling cost 4 more VALU per score in
// kernels that are VALU-bound on the softmax).
// LDS rows of 64 bf16 (128 B) are stored with the 16-byte chunk swizzle chunk ^ g((row >> 1) & 7),
// g(k) = (k >> 1) | ((k & 1) << 2): conflict-free for 32-row ds_read_b128 at one chunk and for the
// 4-row transposed reads.
// Key-padding mask (MASK instances; AttnArgs::km, one row of ceil(N / 32) words per SAMPLE, bit j of word kt
// = key 32 kt + j takes part): a cleared key is handled like a key >= N. In the forward and dq kernels the key
// is the accumulator row, so its bit is tile_bit(w, v, h) of the wave-uniform word km[b * wpr + kt]; in the dkv
// kernel the key is on the lane, bit kl of this wave's word. Probabilities of cleared keys are SELECTED to 0
// (never multiplied by 0: with no key set in a sample lse = -inf and exp2(.. - lse2) = +inf), their dk / dv
// rows are stored as +0, and a sample with no key set gives out = +0, lse = -inf. All N positions stay
// queries. K / V rows of cleared keys must be finite: they enter the MFMAs with weight 0, and 0 * NaN is NaN.
// Tensors are (B, N, H, 64) in memory with the head dimension contiguous: element (b, n, h, c)
// at b * sB + n * sN + h * 64 + c (fused qkv projections and HF's transposed views alike).
// This file holds the kernels and their launches only: the argument struct AttnArgs, the entry points'
// checks and the tile helpers are in attention_tiles.h (shared with the streaming kernels of
// attention_long.hip), the dropout keep words come from attention_mask.hip.
#include "attention_tiles.h"

namespace {

// rows [0, 32 NT) of two (b, h) slices into swizzled LDS, zero rows >= N. Every global load is
// issued before the first LDS write (one latency, not one per row).
template <int NT>
__device__ __forceinline__ void load_rows2(char* l0, const bf16* b0, long long s0, char* l1, const bf16* b1,
                                           long long s1, int N) {
  static_assert((NT * 32 * 8) % 256 == 0, "256 threads");
  constexpr int PER = NT * 32 * 8 / 256;
  bf16x8 r0[PER], r1[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = threadIdx.x + 256 * i, r = e >> 3, c = e & 7;
    r0[i] = r < N ? *(const bf16x8*)(b0 + (long long)r * s0 + c * 8) : (bf16x8){};
    r1[i] = r < N ? *(const bf16x8*)(b1 + (long long)r * s1 + c * 8) : (bf16x8){};
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = threadIdx.x + 256 * i, r = e >> 3, c = e & 7;
    const int off = r * 128 + ((c ^ swz(r)) << 4);
    *(bf16x8*)(l0 + off) = r0[i];
    *(bf16x8*)(l1 + off) = r1[i];
  }
}

// ---------------------------------------------------------------------------------------------
template <int NKT, bool DROP, bool MASK>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2 * NKT * 32 * 128];
  char* kl = lds;
  char* vl = lds + NKT * 32 * 128;
  const int bh = blockIdx.y, b = bh / a.H, hh = bh - b * a.H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, ql = lane & 31;
  // this wave's query fragments are requested before the block's K / V staging, so their
  // latency overlaps it (issued after the barrier they were a second exposed round trip)
  const int qt = blockIdx.x * 4 + wave;
  const int q = qt * 32 + ql;
  const bool qok = q < a.N;
  bf16x8 qf[4];
  {
    const bf16* qp = a.q + b * a.q_sB + (long long)(qok ? q : 0) * a.q_sN + hh * HD + 8 * h;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = qok ? *(const bf16x8*)(qp + 16 * s) : (bf16x8){};
  }
  load_rows2<NKT>(kl, a.k + b * a.k_sB + hh * HD, a.k_sN, vl, a.v + b * a.v_sB + hh * HD, a.v_sN, a.N);
  __syncthreads();
  if (qt * 32 >= a.N) return;
  f32x16 acc[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    acc[kt] = (f32x16){};
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[kt] = mfma32(lds_b128(kl, kt * 32 + ql, 2 * s + h), qf[s], acc[kt]);
  }
  // keys >= N only in the last tile
  const int nlast = a.N - (NKT - 1) * 32;
  if (nlast < 32) {
#pragma unroll
    for (int v = 0; v < 16; ++v)
      if (acc_row(v, h) >= nlast) acc[NKT - 1][v] = -INFINITY;
  }
  if (MASK) {  // cleared keys leave the softmax like the keys >= N (one wave-uniform word per tile)
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const unsigned w = a.km[b * a.wpr + kt];
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[kt][v] = tile_bit(w, v, h) ? acc[kt][v] : -INFINITY;
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int v = 0; v < 16; ++v) m = fmaxf(m, acc[kt][v]);
  m = fmaxf(m, __shfl_xor(m, 32));
  const float c2 = a.scale * LOG2E;
  // a sample with no key set: m = -inf; -mo = +inf would make every argument NaN (0 keeps them -inf: p = 0)
  const float mo = MASK && m == -INFINITY ? 0.f : m * c2;
  float l = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const float p = __builtin_amdgcn_exp2f(fmaf(acc[kt][v], c2, -mo));  // raw v_exp_f32 (arg <= 0)
      acc[kt][v] = p;
      l += p;
    }
  l += __shfl_xor(l, 32);
  if (DROP) {  // O = sum_k p_k keep_k / (1 - p) v_k; l (the normaliser) keeps every p_k
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const unsigned w = qok ? a.wq[((long long)bh * a.N + q) * NKT + kt] : 0u;
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[kt][v] = tile_bit(w, v, h) ? acc[kt][v] : 0.f;
    }
  }

  f32x16 o0 = {}, o1 = {};
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int c = 2 * kt + half;
      const bf16x8 pf = pack8(acc[kt], half);
      o0 = mfma32(frag_tr(vl, c, 0, lane), pf, o0);
      o1 = mfma32(frag_tr(vl, c, 32, lane), pf, o1);
    }
  if (!qok) return;
  if (MASK && l == 0.f) {  // no key set: out = +0 (not 0 / 0), lse = -inf + log 0 = -inf
    o0 = (f32x16){};
    o1 = (f32x16){};
  }
  const float inv = MASK && l == 0.f ? 0.f : (DROP ? a.drop_scale : 1.f) / l;
  bf16* op = a.out + b * a.out_sB + (long long)q * a.out_sN + hh * HD;
  store_cols(op, o0, inv, h);
  store_cols(op + 32, o1, inv, h);
  if (h == 0) a.lse[(long long)bh * a.N + q] = m * a.scale + logf(l);
}

// dQ: wave = query tile, query on the lane (the forward's orientation)
template <int NKT, bool DROP, bool MASK>
__global__ __launch_bounds__(256, 2) void attn_dq_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2 * NKT * 32 * 128];
  char* kl = lds;
  char* vl = lds + NKT * 32 * 128;
  const int bh = blockIdx.y, b = bh / a.H, hh = bh - b * a.H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, ql = lane & 31;
  const int qt = blockIdx.x * 4 + wave;
  const int q = qt * 32 + ql;
  const bool qok = q < a.N;  // (the wave's global loads below are issued before the barrier)
  bf16x8 qf[4], df[4], ov[4];
  {
    const long long qq = qok ? q : 0;
    const bf16* qp = a.q + b * a.q_sB + qq * a.q_sN + hh * HD + 8 * h;
    const bf16* dp = a.dout + b * a.do_sB + qq * a.do_sN + hh * HD + 8 * h;
    const bf16* op = a.o + b * a.o_sB + qq * a.o_sN + hh * HD + 8 * h;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      qf[s] = qok ? *(const bf16x8*)(qp + 16 * s) : (bf16x8){};
      df[s] = qok ? *(const bf16x8*)(dp + 16 * s) : (bf16x8){};
      ov[s] = qok ? *(const bf16x8*)(op + 16 * s) : (bf16x8){};
    }
  }
  const float lse2 = qok ? a.lse[(long long)bh * a.N + q] * LOG2E : 0.f;
  load_rows2<NKT>(kl, a.k + b * a.k_sB + hh * HD, a.k_sN, vl, a.v + b * a.v_sB + hh * HD, a.v_sN, a.N);
  __syncthreads();
  if (qt * 32 >= a.N) return;
  float dl = 0.f;  // D = rowsum(dO * O) of this query: the lane's 32 dims + the other half's
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int i = 0; i < 8; ++i) dl = fmaf((float)df[s][i], (float)ov[s][i], dl);
  dl += __shfl_xor(dl, 32);
  if (qok && h == 0) a.delta[(long long)bh * a.N + q] = dl;  // for the dkv kernel (launched after)
  const float c2 = a.scale * LOG2E;
  f32x16 g0 = {}, g1 = {};
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    f32x16 s = {}, dp = {};
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      s = mfma32(lds_b128(kl, kt * 32 + ql, 2 * st + h), qf[st], s);
      dp = mfma32(lds_b128(vl, kt * 32 + ql, 2 * st + h), df[st], dp);
    }
    const int nv = a.N - kt * 32;
    const unsigned w = DROP && qok ? a.wq[((long long)bh * a.N + q) * NKT + kt] : 0u;
    const unsigned wm = MASK ? a.km[b * a.wpr + kt] : ~0u;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      // (a cleared key, or any key of a sample with none set, where lse = -inf makes e = +inf: selected away)
      const bool ok = qok && acc_row(v, h) < nv && (!MASK || tile_bit(wm, v, h));
      const float e = __builtin_amdgcn_exp2f(fmaf(s[v], c2, -lse2));
      const float p = ok ? e : 0.f;
      const float dpv = DROP ? (tile_bit(w, v, h) ? dp[v] * a.drop_scale : 0.f) : dp[v];
      s[v] = p * (dpv - dl);  // dS
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int c = 2 * kt + half;
      const bf16x8 sf = pack8(s, half);
      g0 = mfma32(frag_tr(kl, c, 0, lane), sf, g0);
      g1 = mfma32(frag_tr(kl, c, 32, lane), sf, g1);
    }
  }
  if (!qok) return;
  bf16* gp = a.dq + b * a.dq_sB + (long long)q * a.dq_sN + hh * HD;
  store_cols(gp, g0, a.scale, h);
  store_cols(gp + 32, g1, a.scale, h);
}

// dK, dV: wave = key tile, key on the lane
template <int NQT, bool DROP, bool MASK>
__global__ __launch_bounds__(256, 2) void attn_dkv_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2 * NQT * 32 * 128];
  __shared__ float stat[2][NQT * 32];
  char* ql_ = lds;
  char* dl_ = lds + NQT * 32 * 128;
  const int bh = blockIdx.y, b = bh / a.H, hh = bh - b * a.H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, kl = lane & 31;
  const int kt = blockIdx.x * 4 + wave;
  const int key = kt * 32 + kl;
  // a cleared key is treated like a key >= N (p = 0 by selection: with no key set lse = -inf and e = +inf),
  // except that its dk / dv rows are written (as +0)
  const unsigned wm = MASK && kt * 32 < a.N ? a.km[b * a.wpr + kt] : ~0u;   // this wave's tile of the sample's word row
  const bool kok = key < a.N && ((wm >> kl) & 1u);
  bf16x8 kf[4], vf[4];  // requested before the block's Q / dO staging (latency overlapped)
  {
    const long long kk = kok ? key : 0;
    const bf16* kp = a.k + b * a.k_sB + kk * a.k_sN + hh * HD + 8 * h;
    const bf16* vp = a.v + b * a.v_sB + kk * a.v_sN + hh * HD + 8 * h;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      kf[s] = kok ? *(const bf16x8*)(kp + 16 * s) : (bf16x8){};
      vf[s] = kok ? *(const bf16x8*)(vp + 16 * s) : (bf16x8){};
    }
  }
  load_rows2<NQT>(ql_, a.q + b * a.q_sB + hh * HD, a.q_sN, dl_, a.dout + b * a.do_sB + hh * HD, a.do_sN, a.N);
  for (int i = threadIdx.x; i < NQT * 32; i += blockDim.x) {
    const bool ok = i < a.N;
    stat[0][i] = ok ? a.lse[(long long)bh * a.N + i] * LOG2E : INFINITY;  // p = 0 past N
    stat[1][i] = ok ? a.delta[(long long)bh * a.N + i] : 0.f;
  }
  __syncthreads();
  if (kt * 32 >= a.N) return;
  const float c2 = a.scale * LOG2E;
  f32x16 dv0 = {}, dv1 = {}, dk0 = {}, dk1 = {};
#pragma unroll 1
  for (int qt = 0; qt < NQT; ++qt) {
    f32x16 s = {}, dp = {};
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      s = mfma32(lds_b128(ql_, qt * 32 + kl, 2 * st + h), kf[st], s);   // S[q][key]: C[row=q][col=key]
      dp = mfma32(lds_b128(dl_, qt * 32 + kl, 2 * st + h), vf[st], dp);
    }
    // rows of this lane's accumulator: queries qt*32 + (v&3) + 8(v>>2) + 4h (4 runs of 4)
    const unsigned w = DROP && kok ? a.wk[((long long)bh * a.N + key) * NQT + qt] : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q0 = qt * 32 + 8 * j + 4 * h;
      const f32x4 ls = *(const f32x4*)&stat[0][q0];
      const f32x4 de = *(const f32x4*)&stat[1][q0];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int v = 4 * j + i;
        const float e = __builtin_amdgcn_exp2f(fmaf(s[v], c2, -ls[i]));
        const float p = kok ? e : 0.f;
        if (DROP) {
          const float m = tile_bit(w, v, h) ? a.drop_scale : 0.f;
          s[v] = p * m;                 // dropped probability (dV operand)
          dp[v] = p * (dp[v] * m - de[i]);  // dS
        } else {
          s[v] = p;
          dp[v] = p * (dp[v] - de[i]);  // dS
        }
      }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int c = 2 * qt + half;
      const bf16x8 pf = pack8(s, half);
      const bf16x8 sf = pack8(dp, half);
      const bf16x8 d0 = frag_tr(dl_, c, 0, lane), d1 = frag_tr(dl_, c, 32, lane);
      const bf16x8 q0 = frag_tr(ql_, c, 0, lane), q1 = frag_tr(ql_, c, 32, lane);
      dv0 = mfma32(pf, d0, dv0);  // dV[key][dim]: A = P^T (key rows), B = dO (query k, dim cols)
      dv1 = mfma32(pf, d1, dv1);
      dk0 = mfma32(sf, q0, dk0);
      dk1 = mfma32(sf, q1, dk1);
    }
  }
  // C[row = key (v&3)+8(v>>2)+4h][col = dim (lane&31)]
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int kr = kt * 32 + acc_row(v, h);
    if (kr < a.N) {
      const bool set = !MASK || tile_bit(wm, v, h);   // rows of cleared keys: +0 by selection
      bf16* dkp = a.dk + b * a.dk_sB + (long long)kr * a.dk_sN + hh * HD + kl;
      bf16* dvp = a.dv + b * a.dv_sB + (long long)kr * a.dv_sN + hh * HD + kl;
      dkp[0] = (bf16)(set ? dk0[v] * a.scale : 0.f);
      dkp[32] = (bf16)(set ? dk1[v] * a.scale : 0.f);
      dvp[0] = (bf16)(set ? dv0[v] : 0.f);
      dvp[32] = (bf16)(set ? dv1[v] : 0.f);
    }
  }
}

// (B, N) bytes (non-zero = keep) -> B x ceil(N / 32) key-mask words: one thread per word, bits of keys >= N zero
__global__ __launch_bounds__(256) void attn_keymask_pack_kernel(const unsigned char* __restrict__ mask, int B, int N,
                                                                int wpr, unsigned* __restrict__ words) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * wpr) return;
  const int b = i / wpr, kt = i - b * wpr;
  const int n = min(32, N - kt * 32);
  const unsigned char* row = mask + (long long)b * N + kt * 32;
  unsigned w = 0u;
  for (int j = 0; j < n; ++j) w |= (row[j] != 0 ? 1u : 0u) << j;
  words[i] = w;
}

#define ATTN_SWITCH_NT(KERNEL, DR, MK, NT, GRID, ARGS)                                              \
  switch (NT) {                                                                                    \
    case 1: hipLaunchKernelGGL((KERNEL<1, DR, MK>), GRID, dim3(256), 0, stream, ARGS); break;       \
    case 2: hipLaunchKernelGGL((KERNEL<2, DR, MK>), GRID, dim3(256), 0, stream, ARGS); break;       \
    case 3: hipLaunchKernelGGL((KERNEL<3, DR, MK>), GRID, dim3(256), 0, stream, ARGS); break;       \
    case 4: hipLaunchKernelGGL((KERNEL<4, DR, MK>), GRID, dim3(256), 0, stream, ARGS); break;       \
    case 5: hipLaunchKernelGGL((KERNEL<5, DR, MK>), GRID, dim3(256), 0, stream, ARGS); break;       \
    case 6: hipLaunchKernelGGL((KERNEL<6, DR, MK>), GRID, dim3(256), 0, stream, ARGS); break;       \
    case 7: hipLaunchKernelGGL((KERNEL<7, DR, MK>), GRID, dim3(256), 0, stream, ARGS); break;       \
    case 8: hipLaunchKernelGGL((KERNEL<8, DR, MK>), GRID, dim3(256), 0, stream, ARGS); break;       \
    case 9: hipLaunchKernelGGL((KERNEL<9, DR, MK>), GRID, dim3(256), 0, stream, ARGS); break;       \
    default: hipLaunchKernelGGL((KERNEL<10, DR, MK>), GRID, dim3(256), 0, stream, ARGS); break;     \
  }
// the instance by (dropout words given, key mask given)
#define ATTN_SWITCH(KERNEL, DROP, MASK, NT, GRID, ARGS)                          \
  if (DROP) {                                                                   \
    if (MASK) { ATTN_SWITCH_NT(KERNEL, true, true, NT, GRID, ARGS) }            \
    else { ATTN_SWITCH_NT(KERNEL, true, false, NT, GRID, ARGS) }                \
  } else {                                                                      \
    if (MASK) { ATTN_SWITCH_NT(KERNEL, false, true, NT, GRID, ARGS) }           \
    else { ATTN_SWITCH_NT(KERNEL, false, false, NT, GRID, ARGS) }               \
  }

static_assert(MAX_N_SHORT == 10 * 32, "ATTN_SWITCH instantiates 1 .. 10 tiles of 32");
}  // namespace

// (the keep words wq / wk come from triad_attn_dropmask, attention_mask.hip; the key-mask words km from
// triad_attn_keymask_pack below)
extern "C" {

int triad_attn_keymask_pack(const void* mask, int B, int N, unsigned* words, hipStream_t stream) {
  if (!mask || !words || ((uintptr_t)words & 3) || B <= 0 || N < 1 || N > MAX_N_SHORT || B > 65535)
    return TRIAD_EINVAL;
  const int wpr = (N + 31) / 32;
  hipLaunchKernelGGL(attn_keymask_pack_kernel, dim3((B * wpr + 255) / 256), dim3(256), 0, stream,
                     (const unsigned char*)mask, B, N, wpr, words);
  TRIAD_CHECK_LAUNCH();
  return TRIAD_OK;
}

int triad_attn_fwd_keymask(const void* q, long long q_sB, long long q_sN, const void* k, long long k_sB,
                           long long k_sN, const void* v, long long v_sB, long long v_sN, int B, int H, int N, int D,
                           float scale, const unsigned* wq, float p, const unsigned* km, void* out, long long out_sB,
                           long long out_sN, float* lse, hipStream_t stream) {
  AttnArgs a = {};
  if (!attn_fwd_args(a, ATTN_SHORT, {q, q_sB, q_sN}, {k, k_sB, k_sN}, {v, v_sB, v_sN}, B, H, N, D, scale, wq, p,
                     {out, out_sB, out_sN}, lse) ||
      ((uintptr_t)km & 3))
    return TRIAD_EINVAL;
  a.km = km;
  const int nt = (N + 31) / 32;
  const dim3 grid = attn_grid(B, H, N);
  ATTN_SWITCH(attn_fwd_kernel, wq, km, nt, grid, a)
  TRIAD_CHECK_LAUNCH();
  return TRIAD_OK;
}

int triad_attn_fwd_dropout(const void* q, long long q_sB, long long q_sN, const void* k, long long k_sB,
                           long long k_sN, const void* v, long long v_sB, long long v_sN, int B, int H, int N, int D,
                           float scale, const unsigned* wq, float p, void* out, long long out_sB, long long out_sN,
                           float* lse, hipStream_t stream) {
  return triad_attn_fwd_keymask(q, q_sB, q_sN, k, k_sB, k_sN, v, v_sB, v_sN, B, H, N, D, scale, wq, p, nullptr, out,
                                out_sB, out_sN, lse, stream);
}

int triad_attn_fwd(const void* q, long long q_sB, long long q_sN, const void* k, long long k_sB, long long k_sN,
                   const void* v, long long v_sB, long long v_sN, int B, int H, int N, int D, float scale, void* out,
                   long long out_sB, long long out_sN, float* lse, hipStream_t stream) {
  return triad_attn_fwd_keymask(q, q_sB, q_sN, k, k_sB, k_sN, v, v_sB, v_sN, B, H, N, D, scale, nullptr, 0.f, nullptr,
                                out, out_sB, out_sN, lse, stream);
}

int triad_attn_bwd_keymask(const void* q, long long q_sB, long long q_sN, const void* k, long long k_sB,
                           long long k_sN, const void* v, long long v_sB, long long v_sN, const void* o,
                           long long o_sB, long long o_sN, const void* dout, long long do_sB, long long do_sN,
                           const float* lse, int B, int H, int N, int D, float scale, const unsigned* wq,
                           const unsigned* wk, float p, const unsigned* km, void* dq, long long dq_sB,
                           long long dq_sN, void* dk, long long dk_sB, long long dk_sN, void* dv, long long dv_sB,
                           long long dv_sN, float* delta, hipStream_t stream) {
  AttnArgs a = {};
  if (!attn_bwd_args(a, ATTN_SHORT, {q, q_sB, q_sN}, {k, k_sB, k_sN}, {v, v_sB, v_sN}, {o, o_sB, o_sN},
                     {dout, do_sB, do_sN}, lse, B, H, N, D, scale, wq, wk, p, {dq, dq_sB, dq_sN}, {dk, dk_sB, dk_sN},
                     {dv, dv_sB, dv_sN}, delta) ||
      ((uintptr_t)km & 3))
    return TRIAD_EINVAL;
  a.km = km;
  const int nt = (N + 31) / 32;
  const dim3 grid = attn_grid(B, H, N);
  ATTN_SWITCH(attn_dq_kernel, wq, km, nt, grid, a)
  ATTN_SWITCH(attn_dkv_kernel, wq, km, nt, grid, a)
  TRIAD_CHECK_LAUNCH();
  return TRIAD_OK;
}

int triad_attn_bwd_dropout(const void* q, long long q_sB, long long q_sN, const void* k, long long k_sB,
                           long long k_sN, const void* v, long long v_sB, long long v_sN, const void* o,
                           long long o_sB, long long o_sN, const void* dout, long long do_sB, long long do_sN,
                           const float* lse, int B, int H, int N, int D, float scale, const unsigned* wq,
                           const unsigned* wk, float p, void* dq, long long dq_sB, long long dq_sN, void* dk,
                           long long dk_sB, long long dk_sN, void* dv, long long dv_sB, long long dv_sN, float* delta,
                           hipStream_t stream) {
  return triad_attn_bwd_keymask(q, q_sB, q_sN, k, k_sB, k_sN, v, v_sB, v_sN, o, o_sB, o_sN, dout, do_sB, do_sN, lse,
                                B, H, N, D, scale, wq, wk, p, nullptr, dq, dq_sB, dq_sN, dk, dk_sB, dk_sN, dv, dv_sB,
                                dv_sN, delta, stream);
}

int triad_attn_bwd(const void* q, long long q_sB, long long q_sN, const void* k, long long k_sB, long long k_sN,
                   const void* v, long long v_sB, long long v_sN, const void* o, long long o_sB, long long o_sN,
                   const void* dout, long long do_sB, long long do_sN, const float* lse, int B, int H, int N, int D,
                   float scale, void* dq, long long dq_sB, long long dq_sN, void* dk, long long dk_sB,
                   long long dk_sN, void* dv, long long dv_sB, long long dv_sN, float* delta, hipStream_t stream) {
  return triad_attn_bwd_keymask(q, q_sB, q_sN, k, k_sB, k_sN, v, v_sB, v_sN, o, o_sB, o_sN, dout, do_sB, do_sN, lse,
                                B, H, N, D, scale, nullptr, nullptr, 0.f, nullptr, dq, dq_sB, dq_sN, dk, dk_sB, dk_sN,
                                dv, dv_sB, dv_sN, delta, stream);
}

}  // extern "C"

