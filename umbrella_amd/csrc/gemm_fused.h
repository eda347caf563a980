// Epilogue selector and optional fused work of the GEMM family (gemm.hip: skinny / verify kernels; vgemm.hip: the wide
// verify kernel of round 6), device-side mirror of include/umbrella_hip.h UmbGemmFused; and the pieces the wide kernels
// share: the exact int4 dequant and the direct epilogue.
#pragma once
#include "common.h"
#include "qkv_epilogue.h"

enum { EPI_PARTIAL = 0, EPI_ROUND = 1, EPI_SILU = 2, EPI_QKV = 3, EPI_RESID = 4 };


// Optional fused work around the GEMM (all pointers may be null).  Passed by value.
//  * ssq_in : [T][ssq_groups] partial sums of squares of the producer's residual stream.  The RMSNorm weight is
//    already folded into x by the producer (x = h * w), the per-token factor rsqrt(mean(h^2) + eps) commutes with
//    the matmul and is applied to the outputs here (epi 1, 2, 3).
//  * epi 3 / 4 with S > 1: every split block publishes its fp32 partial tile, the LAST block to arrive on the
//    n-group's counter sums the S partials in split order (deterministic) and runs the epilogue -- no reduce kernel.
struct GemmFused {
  int ssq_stride;          // row stride of ssq_in (0: ssq_groups)
  int x_fm, out_fm;        // x / the SiLU output in FM (MFMA B-fragment) layout, lowlat.hip: the low-latency schedule's buffers
  const float* ssq_in; int ssq_groups; float ssq_dim; float eps;
  unsigned* counters;
  u16* h; u16* hw; const u16* norm_w; float* ssq_out; int ssq_out_stride;    // epi 4
  QkvDst qkv;                                                                // epi 3
};


// ---- exact fp16 int4 dequant, W = fp16((q - z) * s): bit-identical to what awq_ext.dequantize_weights_cuda produces (the wide
// kernels of gemm.hip and vgemm.hip, stage_compute's AWQ == 2).  ONE copy of this arithmetic.
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

// (a & mask) | magic in ONE VALU op.  gfx9 VOP3 may read a single SGPR/constant, so hipcc splits the pattern into
// v_and + v_or when both constants live in SGPRs; keeping `magic` in a VGPR makes v_and_or_b32 encodable.
__device__ __forceinline__ unsigned and_or(unsigned a, unsigned mask, unsigned magic_v) {
  unsigned r;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(mask), "v"(magic_v));
  return r;
}

// Per weight row, from its metadata dword {fp16 scale, fp16(zero)}: packed scale, -(1024 + z) and -(64 + z) (exact:
// |1024 + z| <= 1039).
struct DeqMeta { h2 s2, nz2, nz16_2; };
__device__ __forceinline__ DeqMeta deq_meta(unsigned mm) {
  const _Float16 sc = __builtin_bit_cast(_Float16, (u16)(mm & 0xffffu));
  const _Float16 zf = __builtin_bit_cast(_Float16, (u16)(mm >> 16));
  DeqMeta m;
  m.s2 = h2{sc, sc};
  const _Float16 nz = -((_Float16)1024.0f + zf), nz16 = -((_Float16)64.0f + zf);
  m.nz2 = h2{nz, nz};
  m.nz16_2 = h2{nz16, nz16};
  return m;
}
// Two weights of an A fragment, in two steps.  Codes: nibbles at mantissa bits 0..3 give fp16(1024 + q), at bits 4..7 (`hi`)
// fp16(1024 + 16 q) -- one shift per packed dword instead of three.  `magic` = F16::MAGIC, pinned in a VGPR by the caller, once
// per call site.  Scale: (q - z) is exact in fp16 either way, then ONE rounding in (q - z) * s.
__device__ __forceinline__ h2 deq_codes(unsigned ws, bool hi, unsigned magic) {
  if (hi) return __builtin_bit_cast(h2, and_or(ws, 0x00F000F0u, magic));
  return __builtin_bit_cast(h2, and_or(ws, 0x000F000Fu, magic));
}
__device__ __forceinline__ unsigned deq_scale(h2 c, bool hi, const DeqMeta& m) {
  const h2 sixteenth = {(_Float16)0.0625f, (_Float16)0.0625f};
  if (hi) return __builtin_bit_cast(unsigned, __builtin_elementwise_fma(c, sixteenth, m.nz16_2) * m.s2);
  return __builtin_bit_cast(unsigned, (c + m.nz2) * m.s2);
}
// dword d (0 .. 3) of the A fragment of packed dword w (8 codes): d >= 2 reads w >> 8, odd d the high nibbles
__device__ __forceinline__ unsigned deq_dword(unsigned w, int d, const DeqMeta& m, unsigned magic) {
  const unsigned ws = (d & 2) ? (w >> 8) : w;
  if (d & 1) return deq_scale(deq_codes(ws, true, magic), true, m);
  return deq_scale(deq_codes(ws, false, magic), false, m);
}
// all four dwords: the four v_and_or first, then the arithmetic (the instruction order the kernels were tuned with)
__device__ __forceinline__ u32x4 deq_frag(unsigned w, const DeqMeta& m, unsigned magic) {
  const unsigned w8 = w >> 8;
  const h2 c0 = deq_codes(w, false, magic), c1 = deq_codes(w, true, magic), c2 = deq_codes(w8, false, magic), c3 = deq_codes(w8, true, magic);
  return u32x4{deq_scale(c0, false, m), deq_scale(c1, true, m), deq_scale(c2, false, m), deq_scale(c3, true, m)};
}

// ---- direct epilogue of the wide kernels (verify_gemm_kernel / _r_kernel / _pp_kernel, vgemm_w_kernel)
// per-token 1/rms of the producer's residual stream (fused RMSNorm consumers only); groups are a multiple of 4
__device__ __forceinline__ float gemm_token_inv(const GemmFused& fx, int tok) {
  float inv = 1.f;
  if (fx.ssq_in) {
    const float* sq = fx.ssq_in + (long)tok * (fx.ssq_stride ? fx.ssq_stride : fx.ssq_groups);
    float a = 0.f;
    for (int q = 0; q < fx.ssq_groups; q += 4) { const f32x4 v = *reinterpret_cast<const f32x4*>(sq + q); a += v[0]; a += v[1]; a += v[2]; a += v[3]; }
    inv = rsqrtf(a / fx.ssq_dim + fx.eps);
  }
  return inv;
}
// One accumulator (lane (j, g): token tok, rows 16 ntile + 4 g ..) of split sp: fp32 partials [S][T][N] (epi 1: scaled and
// rounded to the model dtype), or SiLU(gate) * up in the model dtype, [T][N / 2] (rows interleaved (gate_m, up_m), S = 1)
template <typename P>
__device__ __forceinline__ void gemm_store_direct(f32x4 v, float inv, int epi, float* out, int sp, int T, int tok, int N,
                                                  int ntile, int g) {
  if (epi == EPI_SILU) {
    v *= inv;
    const float g0 = rnd<P>(v[0]), u0 = rnd<P>(v[1]), g1 = rnd<P>(v[2]), u1 = rnd<P>(v[3]);
    u16* act = reinterpret_cast<u16*>(out);
    *reinterpret_cast<unsigned*>(act + (long)tok * (N / 2) + ntile * 8 + g * 2) = pack2<P>(silu_mul<P>(g0, u0), silu_mul<P>(g1, u1));
  } else {
    if (epi == EPI_ROUND) { v *= inv; v[0] = rnd<P>(v[0]); v[1] = rnd<P>(v[1]); v[2] = rnd<P>(v[2]); v[3] = rnd<P>(v[3]); }
    *reinterpret_cast<f32x4*>(out + ((long)sp * T + tok) * N + ntile * 16 + g * 4) = v;
  }
}

// vgemm.hip: the wide (T > 64) int4 verify GEMM, fp16 activations, gemm.hip's tile order and epilogues
extern "C" int umb_vgemm_w_ok(int T, int N, int K, int S, int epi);
int umb_vgemm_w(const void* wp, const void* meta, const u16* x, int ldx, float* out, int T, int N, int K, int S, int epi,
                const GemmFused& fx, hipStream_t st);
