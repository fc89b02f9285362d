// Backbone self-attention for sequences of 321 .. 2048 tokens (DINOv2-L/14 at 518 px: 1374 tokens,
// HuBERT-large on 10 s of audio: 499; BASELINE configuration c5), forward and backward, bf16 in /
// fp32 accumulate, head dim 64. Same tensor convention, MFMA orientation, swizzled LDS rows and
// transposed reads as attention.hip (helpers, the argument struct AttnArgs and the entry points' checks
// in attention_tiles.h; the keep words are written by attention_mask.hip); what differs is that a
// (sample, head) sequence no longer fits in LDS, so the other side of each product is streamed in
// chunks of KC = 64 rows through a two-slot LDS ring. Register-staged: the next chunk's global loads
// are issued before the current chunk's MFMAs and written to the free slot after them, one barrier
// per chunk (the slot written in step c was last read in step c - 1, before that step's barrier).
//   forward : wave = 32-query tile, query on the lane, K / V chunks. Online softmax per query:
//             running max m and mo = fl(m c2); per chunk p = exp2(fma(s, c2, -mo_new)),
//             alpha = exp2(mo_old - mo_new), l = fma(l, alpha, sum p), O *= alpha. The mo of an
//             earlier chunk cancels between its p and the alphas that follow, so every p is
//             relative to the final mo whatever the rounding of each m c2. m starts at -inf
//             (alpha = 0 on the first chunk). Keys >= N of the last chunk are zero rows with their
//             scores set to -inf (p = 0). Writes O and lse = m scale + log l.
//   dq      : wave = query tile, K / V chunks; p from the stored lse, the arithmetic of
//             attn_dq_kernel per key tile; forms delta = rowsum(dO o).
//   dkv     : wave = 32-key tile, key on the lane, Q / dO chunks with their lse log2e and delta in
//             LDS beside them; the arithmetic of attn_dkv_kernel per query tile.
// Every output element is written by one lane, sums run in a fixed order: no atomics, no hand-off
// between workgroups, results bit-identical from run to run.
// Dropout keep bits are stored words as in attention.hip, with wpr = 2 ceil(N / 64) words per row
// (rows padded to whole chunks, so a lane reads the two words of a chunk as one 8-byte load):
// wq[(bh N + q) wpr + kt] (bit j = key 32 kt + j), wk[(bh N + key) wpr + qt] (bit j = query 32 qt + j),
// bits of keys / queries >= N zero.
#include "attention_tiles.h"

namespace {

constexpr int KC = 64;             // rows per streamed chunk (two 32-row MFMA tiles)

// One chunk (KC rows x 64 dims) of two (b, h) slices in flight: 2 x 2 16-byte vectors per thread.
struct Stage {
  bf16x8 a[2], b[2];
};
// rows [r0, r0 + KC) -> registers, zero for rows >= N
__device__ __forceinline__ void stage_load(Stage& s, const bf16* b0, long long s0, const bf16* b1, long long s1, int r0,
                                           int N) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = threadIdx.x + 256 * i, r = r0 + (e >> 3), c = e & 7;
    s.a[i] = r < N ? *(const bf16x8*)(b0 + (long long)r * s0 + c * 8) : (bf16x8){};
    s.b[i] = r < N ? *(const bf16x8*)(b1 + (long long)r * s1 + c * 8) : (bf16x8){};
  }
}
// registers -> the swizzled rows [0, KC) of an LDS slot
__device__ __forceinline__ void stage_store(const Stage& s, char* l0, char* l1) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = threadIdx.x + 256 * i, r = e >> 3, c = e & 7;
    const int off = r * 128 + ((c ^ swz(r)) << 4);
    *(bf16x8*)(l0 + off) = s.a[i];
    *(bf16x8*)(l1 + off) = s.b[i];
  }
}

// ---------------------------------------------------------------------------------------------
template <bool DROP>
__global__ __launch_bounds__(256, 2) void attn_long_fwd_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2][2][KC * 128];   // [slot][K, V]
  const int bh = blockIdx.y, b = bh / a.H, hh = bh - b * a.H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, ql = lane & 31;
  const int qt = blockIdx.x * 4 + wave;
  const int q = qt * 32 + ql;
  const bool qok = q < a.N;
  const bool active = qt * 32 < a.N;   // wave-uniform; idle waves still stage and meet the barriers
  bf16x8 qf[4];
  {
    const bf16* qp = a.q + b * a.q_sB + (long long)(qok ? q : 0) * a.q_sN + hh * HD + 8 * h;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = qok ? *(const bf16x8*)(qp + 16 * s) : (bf16x8){};
  }
  const bf16* kb = a.k + b * a.k_sB + hh * HD;
  const bf16* vb = a.v + b * a.v_sB + hh * HD;
  const int nch = (a.N + KC - 1) / KC;
  Stage st;
  stage_load(st, kb, a.k_sN, vb, a.v_sN, 0, a.N);
  stage_store(st, lds[0][0], lds[0][1]);
  __syncthreads();
  const float c2 = a.scale * LOG2E;
  const unsigned* wrow = DROP ? a.wq + ((long long)bh * a.N + (qok ? q : 0)) * a.wpr : nullptr;
  float m = -INFINITY, mo = -INFINITY, l = 0.f;
  f32x16 o0 = {}, o1 = {};
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    const bool more = c + 1 < nch;
    if (more) stage_load(st, kb, a.k_sN, vb, a.v_sN, (c + 1) * KC, a.N);
    if (active) {
      const char* kl = lds[c & 1][0];
      const char* vl = lds[c & 1][1];
      uint2 w = {};
      if (DROP && qok) w = *(const uint2*)(wrow + 2 * c);
      f32x16 s[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        s[t] = (f32x16){};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) s[t] = mfma32(lds_b128(kl, t * 32 + ql, 2 * ks + h), qf[ks], s[t]);
      }
      const int nv = a.N - c * KC;   // keys >= N only in the last chunk
      if (nv < KC) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v)
            if (t * 32 + acc_row(v, h) >= nv) s[t][v] = -INFINITY;
      }
      float cm = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) cm = fmaxf(cm, s[t][v]);
      cm = fmaxf(cm, __shfl_xor(cm, 32));
      const float mn = fmaxf(m, cm);
      const float mon = mn * c2;
      const float alpha = __builtin_amdgcn_exp2f(mo - mon);   // 0 on the first chunk, 1 if the max stood
      float ls = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[t][v], c2, -mon));  // raw v_exp_f32 (arg <= 0)
          s[t][v] = p;
          ls += p;
        }
      l = fmaf(l, alpha, ls);   // this lane's half of the keys; the halves meet after the loop
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        o0[v] *= alpha;
        o1[v] *= alpha;
      }
      m = mn;
      mo = mon;
      if (DROP) {  // the normaliser keeps every p
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          s[0][v] = tile_bit(w.x, v, h) ? s[0][v] : 0.f;
          s[1][v] = tile_bit(w.y, v, h) ? s[1][v] : 0.f;
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const bf16x8 pf = pack8(s[t], half);
          o0 = mfma32(frag_tr(vl, 2 * t + half, 0, lane), pf, o0);
          o1 = mfma32(frag_tr(vl, 2 * t + half, 32, lane), pf, o1);
        }
    }
    if (more) stage_store(st, lds[(c + 1) & 1][0], lds[(c + 1) & 1][1]);
    __syncthreads();
  }
  if (!active) return;
  l += __shfl_xor(l, 32);
  if (!qok) return;
  const float inv = (DROP ? a.drop_scale : 1.f) / l;
  bf16* op = a.out + b * a.out_sB + (long long)q * a.out_sN + hh * HD;
  store_cols(op, o0, inv, h);
  store_cols(op + 32, o1, inv, h);
  if (h == 0) a.lse[(long long)bh * a.N + q] = m * a.scale + logf(l);
}

// dQ: wave = query tile, query on the lane, K / V chunks
template <bool DROP>
__global__ __launch_bounds__(256, 2) void attn_long_dq_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2][2][KC * 128];   // [slot][K, V]
  const int bh = blockIdx.y, b = bh / a.H, hh = bh - b * a.H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, ql = lane & 31;
  const int qt = blockIdx.x * 4 + wave;
  const int q = qt * 32 + ql;
  const bool qok = q < a.N;
  const bool active = qt * 32 < a.N;
  bf16x8 qf[4], df[4];
  float dl = 0.f;  // D = rowsum(dO * O) of this query: the lane's 32 dims + the other half's
  {
    const long long qq = qok ? q : 0;
    const bf16* qp = a.q + b * a.q_sB + qq * a.q_sN + hh * HD + 8 * h;
    const bf16* dp = a.dout + b * a.do_sB + qq * a.do_sN + hh * HD + 8 * h;
    const bf16* op = a.o + b * a.o_sB + qq * a.o_sN + hh * HD + 8 * h;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      qf[s] = qok ? *(const bf16x8*)(qp + 16 * s) : (bf16x8){};
      df[s] = qok ? *(const bf16x8*)(dp + 16 * s) : (bf16x8){};
      const bf16x8 ov = qok ? *(const bf16x8*)(op + 16 * s) : (bf16x8){};
#pragma unroll
      for (int i = 0; i < 8; ++i) dl = fmaf((float)df[s][i], (float)ov[i], dl);
    }
  }
  dl += __shfl_xor(dl, 32);
  if (qok && h == 0) a.delta[(long long)bh * a.N + q] = dl;  // for the dkv kernel (launched after)
  const float lse2 = qok ? a.lse[(long long)bh * a.N + q] * LOG2E : 0.f;
  const bf16* kb = a.k + b * a.k_sB + hh * HD;
  const bf16* vb = a.v + b * a.v_sB + hh * HD;
  const int nch = (a.N + KC - 1) / KC;
  Stage st;
  stage_load(st, kb, a.k_sN, vb, a.v_sN, 0, a.N);
  stage_store(st, lds[0][0], lds[0][1]);
  __syncthreads();
  const float c2 = a.scale * LOG2E;
  const unsigned* wrow = DROP ? a.wq + ((long long)bh * a.N + (qok ? q : 0)) * a.wpr : nullptr;
  f32x16 g0 = {}, g1 = {};
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    const bool more = c + 1 < nch;
    if (more) stage_load(st, kb, a.k_sN, vb, a.v_sN, (c + 1) * KC, a.N);
    if (active) {
      const char* kl = lds[c & 1][0];
      const char* vl = lds[c & 1][1];
      uint2 w = {};
      if (DROP && qok) w = *(const uint2*)(wrow + 2 * c);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x16 s = {}, dp = {};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          s = mfma32(lds_b128(kl, t * 32 + ql, 2 * ks + h), qf[ks], s);
          dp = mfma32(lds_b128(vl, t * 32 + ql, 2 * ks + h), df[ks], dp);
        }
        const int nv = a.N - c * KC - t * 32;
        const unsigned wt = t ? w.y : w.x;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const bool ok = qok && acc_row(v, h) < nv;
          const float e = __builtin_amdgcn_exp2f(fmaf(s[v], c2, -lse2));
          const float p = ok ? e : 0.f;
          const float dpv = DROP ? (tile_bit(wt, v, h) ? dp[v] * a.drop_scale : 0.f) : dp[v];
          s[v] = p * (dpv - dl);  // dS
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const bf16x8 sf = pack8(s, half);
          g0 = mfma32(frag_tr(kl, 2 * t + half, 0, lane), sf, g0);
          g1 = mfma32(frag_tr(kl, 2 * t + half, 32, lane), sf, g1);
        }
      }
    }
    if (more) stage_store(st, lds[(c + 1) & 1][0], lds[(c + 1) & 1][1]);
    __syncthreads();
  }
  if (!qok) return;
  bf16* gp = a.dq + b * a.dq_sB + (long long)q * a.dq_sN + hh * HD;
  store_cols(gp, g0, a.scale, h);
  store_cols(gp + 32, g1, a.scale, h);
}

// dK, dV: wave = key tile, key on the lane, Q / dO chunks with their lse log2e and delta
template <bool DROP>
__global__ __launch_bounds__(256, 2) void attn_long_dkv_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[2][2][KC * 128];   // [slot][Q, dO]
  __shared__ __attribute__((aligned(16))) float stat[2][2][KC];       // [slot][lse log2e, delta]
  const int bh = blockIdx.y, b = bh / a.H, hh = bh - b * a.H;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, kl = lane & 31;
  const int kt = blockIdx.x * 4 + wave;
  const int key = kt * 32 + kl;
  const bool kok = key < a.N;
  const bool active = kt * 32 < a.N;
  bf16x8 kf[4], vf[4];
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
  const bf16* qb = a.q + b * a.q_sB + hh * HD;
  const bf16* db = a.dout + b * a.do_sB + hh * HD;
  const int nch = (a.N + KC - 1) / KC;
  // threads 0 .. 63 stage lse log2e (inf past N: p = 0), 64 .. 127 delta (0 past N)
  const int sw = threadIdx.x >> 6, sr = threadIdx.x & 63;
  const float* sbase = (sw == 0 ? a.lse : a.delta) + (long long)bh * a.N;
  auto stat_load = [&](int r0) -> float {
    if (sw >= 2) return 0.f;
    const int r = r0 + sr;
    if (sw == 0) return r < a.N ? sbase[r] * LOG2E : INFINITY;
    return r < a.N ? sbase[r] : 0.f;
  };
  Stage st;
  float sv = stat_load(0);
  stage_load(st, qb, a.q_sN, db, a.do_sN, 0, a.N);
  stage_store(st, lds[0][0], lds[0][1]);
  if (sw < 2) stat[0][sw][sr] = sv;
  __syncthreads();
  const float c2 = a.scale * LOG2E;
  const unsigned* wrow = DROP ? a.wk + ((long long)bh * a.N + (kok ? key : 0)) * a.wpr : nullptr;
  f32x16 dv0 = {}, dv1 = {}, dk0 = {}, dk1 = {};
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    const bool more = c + 1 < nch;
    if (more) {
      stage_load(st, qb, a.q_sN, db, a.do_sN, (c + 1) * KC, a.N);
      sv = stat_load((c + 1) * KC);
    }
    if (active) {
      const char* ql_ = lds[c & 1][0];
      const char* dl_ = lds[c & 1][1];
      uint2 w = {};
      if (DROP && kok) w = *(const uint2*)(wrow + 2 * c);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x16 s = {}, dp = {};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          s = mfma32(lds_b128(ql_, t * 32 + kl, 2 * ks + h), kf[ks], s);   // S[q][key]: C[row=q][col=key]
          dp = mfma32(lds_b128(dl_, t * 32 + kl, 2 * ks + h), vf[ks], dp);
        }
        const unsigned wt = t ? w.y : w.x;
        // rows of this lane's accumulator: queries c KC + 32 t + (v&3) + 8(v>>2) + 4h (4 runs of 4)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int q0 = t * 32 + 8 * j + 4 * h;
          const f32x4 ls = *(const f32x4*)&stat[c & 1][0][q0];
          const f32x4 de = *(const f32x4*)&stat[c & 1][1][q0];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int v = 4 * j + i;
            const float e = __builtin_amdgcn_exp2f(fmaf(s[v], c2, -ls[i]));
            const float p = kok ? e : 0.f;
            if (DROP) {
              const float mk = tile_bit(wt, v, h) ? a.drop_scale : 0.f;
              s[v] = p * mk;                     // dropped probability (dV operand)
              dp[v] = p * (dp[v] * mk - de[i]);  // dS
            } else {
              s[v] = p;
              dp[v] = p * (dp[v] - de[i]);  // dS
            }
          }
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int cc = 2 * t + half;
          const bf16x8 pf = pack8(s, half);
          const bf16x8 sf = pack8(dp, half);
          const bf16x8 d0 = frag_tr(dl_, cc, 0, lane), d1 = frag_tr(dl_, cc, 32, lane);
          const bf16x8 q0 = frag_tr(ql_, cc, 0, lane), q1 = frag_tr(ql_, cc, 32, lane);
          dv0 = mfma32(pf, d0, dv0);  // dV[key][dim]: A = P^T (key rows), B = dO (query k, dim cols)
          dv1 = mfma32(pf, d1, dv1);
          dk0 = mfma32(sf, q0, dk0);
          dk1 = mfma32(sf, q1, dk1);
        }
      }
    }
    if (more) {
      stage_store(st, lds[(c + 1) & 1][0], lds[(c + 1) & 1][1]);
      if (sw < 2) stat[(c + 1) & 1][sw][sr] = sv;
    }
    __syncthreads();
  }
  if (!active) return;
  // C[row = key (v&3)+8(v>>2)+4h][col = dim (lane&31)]
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int kr = kt * 32 + acc_row(v, h);
    if (kr < a.N) {
      bf16* dkp = a.dk + b * a.dk_sB + (long long)kr * a.dk_sN + hh * HD + kl;
      bf16* dvp = a.dv + b * a.dv_sB + (long long)kr * a.dv_sN + hh * HD + kl;
      dkp[0] = (bf16)(dk0[v] * a.scale);
      dkp[32] = (bf16)(dk1[v] * a.scale);
      dvp[0] = (bf16)dv0[v];
      dvp[32] = (bf16)dv1[v];
    }
  }
}

}  // namespace

// (the keep words wq / wk come from triad_attn_long_dropmask, attention_mask.hip)
extern "C" {

int triad_attn_long_fwd(const void* q, long long q_sB, long long q_sN, const void* k, long long k_sB, long long k_sN,
                        const void* v, long long v_sB, long long v_sN, int B, int H, int N, int D, float scale,
                        const unsigned* wq, float p, void* out, long long out_sB, long long out_sN, float* lse,
                        hipStream_t stream) {
  AttnArgs a = {};
  if (!attn_fwd_args(a, ATTN_LONG, {q, q_sB, q_sN}, {k, k_sB, k_sN}, {v, v_sB, v_sN}, B, H, N, D, scale, wq, p,
                     {out, out_sB, out_sN}, lse))
    return TRIAD_EINVAL;
  const dim3 grid = attn_grid(B, H, N);
  if (wq) hipLaunchKernelGGL(attn_long_fwd_kernel<true>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(attn_long_fwd_kernel<false>, grid, dim3(256), 0, stream, a);
  TRIAD_CHECK_LAUNCH();
  return TRIAD_OK;
}

int triad_attn_long_bwd(const void* q, long long q_sB, long long q_sN, const void* k, long long k_sB, long long k_sN,
                        const void* v, long long v_sB, long long v_sN, const void* o, long long o_sB, long long o_sN,
                        const void* dout, long long do_sB, long long do_sN, const float* lse, int B, int H, int N,
                        int D, float scale, const unsigned* wq, const unsigned* wk, float p, void* dq, long long dq_sB,
                        long long dq_sN, void* dk, long long dk_sB, long long dk_sN, void* dv, long long dv_sB,
                        long long dv_sN, float* delta, hipStream_t stream) {
  AttnArgs a = {};
  if (!attn_bwd_args(a, ATTN_LONG, {q, q_sB, q_sN}, {k, k_sB, k_sN}, {v, v_sB, v_sN}, {o, o_sB, o_sN},
                     {dout, do_sB, do_sN}, lse, B, H, N, D, scale, wq, wk, p, {dq, dq_sB, dq_sN}, {dk, dk_sB, dk_sN},
                     {dv, dv_sB, dv_sN}, delta))
    return TRIAD_EINVAL;
  const dim3 grid = attn_grid(B, H, N);
  if (wq) {
    hipLaunchKernelGGL(attn_long_dq_kernel<true>, grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(attn_long_dkv_kernel<true>, grid, dim3(256), 0, stream, a);
  } else {
    hipLaunchKernelGGL(attn_long_dq_kernel<false>, grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(attn_long_dkv_kernel<false>, grid, dim3(256), 0, stream, a);
  }
  TRIAD_CHECK_LAUNCH();
  return TRIAD_OK;
}

}  // extern "C"
