// The q/k/v and residual epilogues of every GEMM family, written once: rotate-half RoPE in the model dtype, the routing of an
// output row to q / the K cache / the V^T cache, the packed-row order of q / k heads and the 4-wide residual step.  Callers:
// skinny_gemm_kernel, ll_gemm_kernel, gv_kernel, repack_rows_kernel, draft_chain_kernel's tail, reduce_qkv_rope_kernel,
// reduce_qkv_rope_qknorm_kernel, rope_inplace_kernel: they must agree bit for bit (tests/test_qkv_epilogue_exact.py, test_chain.py).
// A caller does itself what differs between the families: its loads (cos / sin, bias, the residual row -- gemv.hip and chain.hip
// issue them at kernel start, so the helpers take VALUES), the bias add, 1/rms and the rounding of the projection to the model
// dtype.  Not in common.h: attn.hip, sample.hip and tp.hip include that one.
#pragma once
#include "common.h"

// Where a q/k/v epilogue reads its positions and tables and writes its rows; a member of the by-value argument structs (never
// SGPR-preloaded, so the kernels do not care about the member order -- but the initialisers are POSITIONAL: qkv_dst below, the
// chain's tail and the two reduce kernels of epilogue.hip list the members in this order, and a swap among the four ints would
// compile).  rope_heads is Hq + Hkv, derived where needed.  qkv_dst fills it from any of the C argument structs of
// include/umbrella_hip.h (UmbGemmFused, UmbGemmLL, UmbChain: the same member names).
struct QkvDst { const int* pos; const int* slot; const u16* cosT; const u16* sinT; u16* q_out; u16* kc; u16* vt; int Hq, Hkv, D, Lmax; };
template <typename C> static inline QkvDst qkv_dst(const C& c) {
  return QkvDst{c.pos, c.slot, (const u16*)c.cosT, (const u16*)c.sinT, (u16*)c.q_out, (u16*)c.k_cache, (u16*)c.vt_cache,
                c.Hq, c.Hkv, c.D, c.Lmax};
}

// packed row n of a [q | k | v] stack <- HF feature (repack mode 2; inverse use: bias lookup): inside each of the rope_heads
// leading heads of size D rows (2m, 2m+1) <- (m, m + D/2), so that RoPE partners are adjacent rows
__host__ __device__ __forceinline__ int qk_rowmap(int n, int D, int rope_heads) {
  const int head = n / D, dp = n % D;
  if (head >= rope_heads) return n;
  return head * D + ((dp & 1) ? (dp >> 1) + D / 2 : (dp >> 1));
}

// ---- rotate-half RoPE of one partner pair (a, b) = features (m, m + D/2): operands are fp32 values of the model dtype, results
// its bits.  x * cos + rotate_half(x) * sin with every product and the sum rounded to the model dtype, as eager torch does
// (apply_rotary_pos_emb, model_utils.py:50-51).  The low half SUBTRACTS rnd(b * sin) instead of adding rnd(-b * sin): the same IEEE
// value, zero signs included, but for fp16 hipcc turns the negated product into an FMA with a +0 addend, so a -0 product became
// +0 where eager torch and the bf16 kernels give -0.  Two functions, because the order of the rounded products is an order of
// instructions (mul_rnd is opaque): the two-pair sites compute both low halves first, as tuned (pair by pair costs two VGPRs).
template <typename P> __device__ __forceinline__ u16 rope_lo(float a, float b, float cos_lo, float sin_lo) {
  return P::from_f(mul_rnd<P>(a, cos_lo) - mul_rnd<P>(b, sin_lo));
}
template <typename P> __device__ __forceinline__ u16 rope_hi(float a, float b, float cos_hi, float sin_hi) {
  return P::from_f(mul_rnd<P>(b, cos_hi) + mul_rnd<P>(a, sin_hi));
}
struct RopePair { u16 lo, hi; };
template <typename P>
__device__ __forceinline__ RopePair rope_rotate(float a, float b, float cos_lo, float cos_hi, float sin_lo, float sin_hi) {
  return RopePair{rope_lo<P>(a, b, cos_lo, sin_lo), rope_hi<P>(a, b, cos_hi, sin_hi)};      // braces: evaluated left to right
}

// ---- destination routing: head of the [q | k | v] stack -> q row of token row t (row-major [T][Hq][D]), or the kv head's K /
// V^T slab, whose elements are addressed in fragment order (common.h kc_off / vt_off) at key slot
__device__ __forceinline__ u16* qkv_q_row(const QkvDst& q, int t, int head) { return q.q_out + ((long)t * q.Hq + head) * q.D; }
__device__ __forceinline__ u16* qkv_k_slab(const QkvDst& q, int head) { return q.kc + (long)(head - q.Hq) * q.Lmax * q.D; }
__device__ __forceinline__ u16* qkv_v_slab(const QkvDst& q, int h) { return q.vt + (long)(h - q.Hq - q.Hkv) * q.D * VT_LD(q.Lmax); }
// one rotated pair (m, m + D/2) of a q / k head as 2-byte stores (gemv, chain, the reduce kernels)
__device__ __forceinline__ void qk_store_pair(const QkvDst& q, int head, int m, int t, int slot, RopePair r) {
  const int D = q.D, half = D / 2;
  if (head < q.Hq) {
    u16* dst = qkv_q_row(q, t, head);
    dst[m] = r.lo;
    dst[m + half] = r.hi;
  } else {
    u16* dst = qkv_k_slab(q, head);
    dst[kc_off(slot, m, D)] = r.lo;
    dst[kc_off(slot, m + half, D)] = r.hi;
  }
}
// two adjacent rotated pairs (m, m + 1; m even, so each half stays one 4-byte store in both layouts) (gemm, lowlat)
__device__ __forceinline__ void qk_store_pairs2(const QkvDst& q, int head, int m, int t, int slot, u16 lo0, u16 lo1, u16 hi0,
                                                u16 hi1) {
  const int D = q.D, half = D / 2;
  u16* dlo = (head < q.Hq) ? qkv_q_row(q, t, head) + m : qkv_k_slab(q, head) + kc_off(slot, m, D);
  u16* dhi = (head < q.Hq) ? dlo + half : qkv_k_slab(q, head) + kc_off(slot, m + half, D);
  *reinterpret_cast<unsigned*>(dlo) = (unsigned)lo0 | ((unsigned)lo1 << 16);
  *reinterpret_cast<unsigned*>(dhi) = (unsigned)hi0 | ((unsigned)hi1 << 16);
}
// v rows (already rounded to the model dtype): features (d0, d1), or the four features d .. d + 3, of a v head at key slot
template <typename P>
__device__ __forceinline__ void v_store2(const QkvDst& q, int head, int d0, int d1, int slot, float v0, float v1) {
  u16* dst = qkv_v_slab(q, head);
  dst[vt_off(d0, slot, q.D)] = P::from_f(v0);
  dst[vt_off(d1, slot, q.D)] = P::from_f(v1);
}
template <typename P>
__device__ __forceinline__ void v_store4(const QkvDst& q, int head, int d, int slot, float v0, float v1, float v2, float v3) {
  v_store2<P>(q, head, d, d + 1, slot, v0, v1);
  v_store2<P>(q, head, d + 2, d + 3, slot, v2, v3);
}

// ---- residual step on four adjacent columns n .. n + 3 of one token (the MFMA kernels; gv_kernel and the chain keep their scalar
// step, whose fma order is pinned separately): h <- rnd(rnd(v) + h) in place at h4; hw4 <- h * norm_w[n ..] (the next RMSNorm's
// weight, folded; skipped when norm_w is null; hw4 is the caller's address, row-major or FM).  Returns the lane's sum of h^2.
template <typename P> __device__ __forceinline__ float resid_step4(f32x4 v, u16* h4, const u16* norm_w, int n, u16* hw4) {
  const uint2 hr = *reinterpret_cast<const uint2*>(h4);
  const float h0 = rnd<P>(rnd<P>(v[0]) + lo_f<P>(hr.x)), h1 = rnd<P>(rnd<P>(v[1]) + hi_f<P>(hr.x));
  const float h2v = rnd<P>(rnd<P>(v[2]) + lo_f<P>(hr.y)), h3 = rnd<P>(rnd<P>(v[3]) + hi_f<P>(hr.y));
  uint2 o;
  o.x = pack2<P>(h0, h1); o.y = pack2<P>(h2v, h3);
  *reinterpret_cast<uint2*>(h4) = o;
  if (norm_w) {
    const uint2 w = *reinterpret_cast<const uint2*>(norm_w + n);
    uint2 ow;
    ow.x = pack2<P>(h0 * lo_f<P>(w.x), h1 * hi_f<P>(w.x)); ow.y = pack2<P>(h2v * lo_f<P>(w.y), h3 * hi_f<P>(w.y));
    *reinterpret_cast<uint2*>(hw4) = ow;
  }
  return h0 * h0 + h1 * h1 + h2v * h2v + h3 * h3;
}
