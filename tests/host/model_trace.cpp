// Launch-trace harness for umbrella_amd/csrc/model.hip (tests/test_model_schedule.py).
//
// model.hip is host code only: it decides which launches a forward issues and with which operands.  This program links the
// host-only object of model.hip against logging stubs of everything it calls -- the 31 umb_* callees and five HIP runtime
// calls -- and drives every entry point through a table of cases.  Each stub prints its name and every argument, so stdout
// is the exact ordered launch list of each forward; the test compares it byte for byte with tests/golden/
// model_schedule_trace.txt.  No GPU, no HIP runtime: device pointers are distinct integers that nothing dereferences.
//
//   model_trace --groups             the case groups, one per line (a group = one setting of model.hip's cached getenv knobs,
//                                    so each group runs in a process of its own)
//   model_trace GROUP                run the group's cases, trace on stdout
//   model_trace --time CASE N        N forwards of one case with silent stubs; prints nanoseconds per forward
#include "../../include/umbrella_hip.h"
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// ------------------------------------------------------------------ printing
static bool g_quiet = false;
static void put(const void* p) { printf(" %lx", (unsigned long)(uintptr_t)p); }        // pointers in hex; NULL prints as 0
static void put(int v) { printf(" %d", v); }
static void put(long v) { printf(" %ld", v); }
static void put(unsigned long v) { printf(" %lu", v); }
static void put(float v) { printf(" %.9g", v); }
static void put(const char* s) { printf(" %s", s); }
// struct arguments: every non-zero field by name (a field that is absent is zero / NULL), or - for a NULL struct
#define FP(f) if (x->f) { printf(" " #f "="); printf("%lx", (unsigned long)(uintptr_t)x->f); }
#define FI(f) if (x->f) printf(" " #f "=%d", (int)x->f);
#define FF(f) if (x->f != 0.f) printf(" " #f "=%.9g", (double)x->f);
static void put(const UmbGemmFused* x) {
  if (!x) { printf(" -"); return; }
  printf(" fused{");
  FP(ssq_in) FI(ssq_groups) FF(ssq_dim) FF(eps) FI(pad0) FP(counters) FP(h) FP(hw) FP(norm_w) FP(ssq_out) FI(ssq_out_stride)
  FI(pad1) FP(pos) FP(slot) FP(cosT) FP(sinT) FP(q_out) FP(k_cache) FP(vt_cache) FI(Hq) FI(Hkv) FI(D) FI(Lmax)
  printf(" }");
}
static void put(const UmbGemmLL* x) {
  if (!x) { printf(" -"); return; }
  printf(" ll{");
  FI(row_from) FI(round_out) FP(ssq_in) FI(ssq_groups) FI(ssq_in_stride) FF(ssq_dim) FF(eps) FP(h) FP(hw) FP(norm_w) FP(ssq_out)
  FI(ssq_out_stride) FI(pad0) FP(pos) FP(slot) FP(cosT) FP(sinT) FP(q_out) FP(k_cache) FP(vt_cache) FP(bias) FI(Hq) FI(Hkv) FI(D)
  FI(Lmax)
  printf(" }");
}
static void put(const UmbChain* x) {
  if (!x) { printf(" -"); return; }
  printf(" chain{");
  FP(w_o) FP(w_gu) FP(w_down) FP(w_qkv) FP(attn) FP(h) FP(hw) FP(ssq) FP(norm2) FP(next_norm) FP(pos) FP(slot) FP(cosT) FP(sinT)
  FP(q_out) FP(k_cache) FP(vt_cache) FP(xchg) FI(T) FI(Tmax) FI(front) FI(tail) FI(H) FI(I) FI(NQKV) FI(ssq_stride)
  FI(ssq_groups_in) FI(Hq) FI(Hkv) FI(D) FI(Lmax) FF(eps)
  printf(" }");
}
template <class... A>
static int call(const char* name, A... a) {
  if (g_quiet) return 0;
  printf("%s", name);
  (put(a), ...);
  printf("\n");
  return 0;
}
// a predicate: its arguments and the answer it gave.  Predicates are pure and launch nothing, so a case shows each distinct
// question once (eff_s alone asks umb_gemm_wide_split some eight times per layer); how often and when model.hip asks is not pinned
static char g_asked[64][96];
static int g_nasked;
template <class... A>
static int pred(int ret, const char* name, A... a) {
  if (g_quiet) return ret;
  char q[96];
  int n = snprintf(q, sizeof q, "%s", name);
  ((n += snprintf(q + n, sizeof q - n, " %d", a)), ...);
  for (int i = 0; i < g_nasked; ++i)
    if (!strcmp(g_asked[i], q)) return ret;
  if (g_nasked < 64) strcpy(g_asked[g_nasked++], q);
  printf("%s -> %d\n", q, ret);
  return ret;
}

static const UmbTPPeer* g_peer;   // the one peer descriptor (real host memory: printed by name, not by address)
static const char* peer_name(const UmbTPPeer* p) { return !p ? "-" : p == g_peer ? "peer" : "?"; }

// ------------------------------------------------------------------ stub rules the cases switch
static int g_ll_wn = 4;           // umb_ll_plan: WN
static int g_gemv_ok = 1;         // umb_gemv_ok answers this for T <= 4
static int g_chain_ok = 1;        // umb_chain_ok answers this for T <= 3 without a bias
static int g_head_stream = 0;     // umb_head_stream_ok answers this for rows <= 8
static int g_hook_rc = 0;         // what the all-reduce hook returns
static int g_hip_fail_at = 0;     // the n-th HIP runtime call from now fails (0: none)
static int hip_rc() { return (g_hip_fail_at > 0 && --g_hip_fail_at == 0) ? 1 : 0; }

extern "C" {
// ---- predicates.  Fixed rules, not the library's: parent and result are compared under the same stubs.
// the plan's S up to 64 rows, at most 2 beyond
int umb_gemm_wide_split(int T, int N, int S) { return pred(T <= 64 ? S : (S > 2 ? 2 : S), "umb_gemm_wide_split", T, N, S); }
// R = 1, WN = g_ll_wn, WK = 2, NW = 8 whatever the shape
void umb_ll_plan(int N, int K, int awq, int* R, int* WN, int* WK, int* NW) {
  *R = 1; *WN = g_ll_wn; *WK = 2; *NW = 8;
  pred(g_ll_wn, "umb_ll_plan", N, K, awq);
}
// the library's own rule: tiles of 16 rows, 3 rounded up to 4
int umb_ll_token_tiles(int T) { return pred(T < 1 || T > 64 ? 0 : T <= 16 ? 1 : T <= 32 ? 2 : 4, "umb_ll_token_tiles", T); }
int umb_gemv_ok(int T, int N, int K, int epi) { return pred(T <= 4 ? g_gemv_ok : 0, "umb_gemv_ok", T, N, K, epi); }
// one group per 128 output rows
int umb_gemv_groups(int T, int N, int K) { return pred(N / 128, "umb_gemv_groups", T, N, K); }
int umb_chain_ok(int T, int H, int I, int NQKV, int D, int has_bias) {
  return pred(T <= 3 && !has_bias ? g_chain_ok : 0, "umb_chain_ok", T, H, I, NQKV, D, has_bias);
}
int umb_head_stream_ok(int rows, int V, int H) { return pred(rows <= 8 ? g_head_stream : 0, "umb_head_stream_ok", rows, V, H); }

// ---- launches
int umb_gemm_fused(void* out, const void* x, int ldx, const void* w, const void* meta, int T, int N, int K, int awq, int S, int R,
                   int epi, const UmbGemmFused* fx, int dtype, umb_stream_t st) {
  return call("umb_gemm_fused", out, x, ldx, w, meta, T, N, K, awq, S, R, epi, fx, dtype, st);
}
int umb_gemm_ll(void* out, const void* x, const void* w, const void* meta, int T, int N, int K, int awq, int epi,
                const UmbGemmLL* fx, int dtype, umb_stream_t st) {
  return call("umb_gemm_ll", out, x, w, meta, T, N, K, awq, epi, fx, dtype, st);
}
int umb_gemv(void* out, const void* x, const void* w_rows, int T, int N, int K, int epi, const UmbGemmLL* fx, int dtype,
             umb_stream_t st) {
  return call("umb_gemv", out, x, w_rows, T, N, K, epi, fx, dtype, st);
}
int umb_draft_chain(const UmbChain* c, int dtype, umb_stream_t st) { return call("umb_draft_chain", c, dtype, st); }
int umb_head_stream(float* logits, const void* x, const float* ssq, int ssq_stride, int groups, float eps, const void* w_rows,
                    int rows, int V, int H, int x_fm_tt, int dtype, umb_stream_t st) {
  return call("umb_head_stream", logits, x, ssq, ssq_stride, groups, eps, w_rows, rows, V, H, x_fm_tt, dtype, st);
}
int umb_embed_ll(void* h, const void* table, int H, int V, int Lmax, int T, const int* tok, const int* pos, const int* slot,
                 const int* prefix, const int* tokens_all, const int* n_ptr, int off, const int* depth, int* pos_out,
                 int* slot_out, int* prefix_out, void* hw_fm, const void* norm_w, float* ssq, int ssq_stride, int dtype,
                 umb_stream_t st) {
  return call("umb_embed_ll", h, table, H, V, Lmax, T, tok, pos, slot, prefix, tokens_all, n_ptr, off, depth, pos_out, slot_out,
              prefix_out, hw_fm, norm_w, ssq, ssq_stride, dtype, st);
}
int umb_embed_prep(void* x, const void* table, int H, int T, const int* tok, const int* pos, const int* slot, const int* prefix,
                   const int* tokens_all, const int* n_ptr, int off, const int* depth, int* pos_out, int* slot_out,
                   int* prefix_out, void* hw, const void* norm_w, float* ssq, int ssq_stride, int dtype, umb_stream_t st) {
  return call("umb_embed_prep", x, table, H, T, tok, pos, slot, prefix, tokens_all, n_ptr, off, depth, pos_out, slot_out,
              prefix_out, hw, norm_w, ssq, ssq_stride, dtype, st);
}
int umb_embed_prep_fm(void* x, const void* table, int H, int T, const int* tok, const int* pos, const int* slot,
                      const int* prefix, const int* tokens_all, const int* n_ptr, int off, const int* depth, int* pos_out,
                      int* slot_out, int* prefix_out, void* hw, const void* norm_w, float* ssq, int ssq_stride, int hw_fm_tt,
                      int dtype, umb_stream_t st) {
  return call("umb_embed_prep_fm", x, table, H, T, tok, pos, slot, prefix, tokens_all, n_ptr, off, depth, pos_out, slot_out,
              prefix_out, hw, norm_w, ssq, ssq_stride, hw_fm_tt, dtype, st);
}
int umb_rmsnorm_fm(void* out, const void* x, const void* w, float eps, int rows, int H, int fm_tt, int dtype, umb_stream_t st) {
  return call("umb_rmsnorm_fm", out, x, w, eps, rows, H, fm_tt, dtype, st);
}
int umb_reduce_residual_norm_fm(const void* partial, int S, int T, int N, const void* residual, void* h_out, void* xn_out,
                                const void* w, float eps, int xn_fm_tt, int dtype, umb_stream_t st) {
  return call("umb_reduce_residual_norm_fm", partial, S, T, N, residual, h_out, xn_out, w, eps, xn_fm_tt, dtype, st);
}
int umb_reduce_residual_hw(const void* partial, int S, int T, int N, const void* residual, void* h_out, void* hw_out,
                           const void* w, float* ssq_out, int ssq_stride, int hw_fm_tt, int dtype, umb_stream_t st) {
  return call("umb_reduce_residual_hw", partial, S, T, N, residual, h_out, hw_out, w, ssq_out, ssq_stride, hw_fm_tt, dtype, st);
}
int umb_reduce_qkv_rope(const void* partial, int S, int T, int Hq, int Hkv, int D, int Lmax, const int* pos, const int* slot,
                        const void* cosT, const void* sinT, void* q_out, void* k_cache, void* vt_cache, int paired,
                        const void* bias, int dtype, umb_stream_t st) {
  return call("umb_reduce_qkv_rope", partial, S, T, Hq, Hkv, D, Lmax, pos, slot, cosT, sinT, q_out, k_cache, vt_cache, paired,
              bias, dtype, st);
}
int umb_reduce_qkv_rope2(const void* partial, int S, int T, int Hq, int Hkv, int D, int Lmax, const int* pos, const int* slot,
                         const void* cosT, const void* sinT, void* q_out, void* k_cache, void* vt_cache, int paired,
                         const void* bias, const float* ssq_in, int ssq_groups, int ssq_stride, float ssq_dim, float eps,
                         int dtype, umb_stream_t st) {
  return call("umb_reduce_qkv_rope2", partial, S, T, Hq, Hkv, D, Lmax, pos, slot, cosT, sinT, q_out, k_cache, vt_cache, paired,
              bias, ssq_in, ssq_groups, ssq_stride, ssq_dim, eps, dtype, st);
}
int umb_reduce_qkv_rope_qknorm(const void* partial, int S, int T, int Hq, int Hkv, int D, int Lmax, const int* pos,
                               const int* slot, const void* cosT, const void* sinT, void* q_out, void* k_cache, void* vt_cache,
                               int paired, const void* bias, const float* ssq_in, int ssq_groups, int ssq_stride, float ssq_dim,
                               float eps, const void* q_norm, const void* k_norm, float qk_eps, int dtype, umb_stream_t st) {
  return call("umb_reduce_qkv_rope_qknorm", partial, S, T, Hq, Hkv, D, Lmax, pos, slot, cosT, sinT, q_out, k_cache, vt_cache,
              paired, bias, ssq_in, ssq_groups, ssq_stride, ssq_dim, eps, q_norm, k_norm, qk_eps, dtype, st);
}
int umb_tree_attn(void* out, const void* q, const void* k_cache, const void* vt_cache, void* po, void* pml, const int* prefix_len,
                  const void* mask_bits, int mask_words, int n_mask_keys, int T, int Hq, int Hkv, int D, int Lmax, int chunk,
                  int max_splits, float scale, uint32_t* counters, int dtype, umb_stream_t st) {
  return call("umb_tree_attn", out, q, k_cache, vt_cache, po, pml, prefix_len, mask_bits, mask_words, n_mask_keys, T, Hq, Hkv, D,
              Lmax, chunk, max_splits, scale, counters, dtype, st);
}
int umb_tree_attn2(void* out, const void* q, const void* k_cache, const void* vt_cache, void* po, void* pml,
                   const int* prefix_len, const void* mask_bits, int mask_words, int n_mask_keys, int T, int Hq, int Hkv, int D,
                   int Lmax, int chunk, int max_splits, float scale, uint32_t* counters, int out_fm_tt, int dtype,
                   umb_stream_t st) {
  return call("umb_tree_attn2", out, q, k_cache, vt_cache, po, pml, prefix_len, mask_bits, mask_words, n_mask_keys, T, Hq, Hkv,
              D, Lmax, chunk, max_splits, scale, counters, out_fm_tt, dtype, st);
}
int umb_tree_attn_gemma2(void* out, const void* q, const void* k_cache, const void* vt_cache, void* po, void* pml,
                         const int* prefix_len, const void* mask_bits, int mask_words, int n_mask_keys, int T, int Hq, int Hkv,
                         int D, int Lmax, int max_splits, float scale, float softcap, const int* pos, int window,
                         uint32_t* counters, int dtype, umb_stream_t st) {
  return call("umb_tree_attn_gemma2", out, q, k_cache, vt_cache, po, pml, prefix_len, mask_bits, mask_words, n_mask_keys, T, Hq,
              Hkv, D, Lmax, max_splits, scale, softcap, pos, window, counters, dtype, st);
}
int umb_sum_splits(float* partial, int S, int64_t n, umb_stream_t st) { return call("umb_sum_splits", partial, S, (long)n, st); }
int umb_tp_publish(const UmbTPPeer* peer, const float* partial, int S, int64_t n, umb_stream_t st) {
  return call("umb_tp_publish", peer_name(peer), partial, S, (long)n, st);
}
int umb_tp_reduce_residual_norm(const UmbTPPeer* peer, int T, int N, const void* residual, void* h_out, void* xn_out,
                                const void* w, float eps, int dtype, umb_stream_t st) {
  return call("umb_tp_reduce_residual_norm", peer_name(peer), T, N, residual, h_out, xn_out, w, eps, dtype, st);
}
int umb_gemma_rmsnorm(void* out, void* x, const void* w, float eps, float scale, int rows, int H, int dtype, umb_stream_t st) {
  return call("umb_gemma_rmsnorm", out, x, w, eps, scale, rows, H, dtype, st);
}
int umb_gemma_sandwich(const float* partial, int S, int T, int H, void* h, void* xn_out, const void* w_post, const void* w_next,
                       float eps, int dtype, umb_stream_t st) {
  return call("umb_gemma_sandwich", partial, S, T, H, h, xn_out, w_post, w_next, eps, dtype, st);
}
int umb_reduce_gelu_mul(const void* partial, int S, int T, int I, void* act, int dtype, umb_stream_t st) {
  return call("umb_reduce_gelu_mul", partial, S, T, I, act, dtype, st);
}
int umb_logit_softcap(float* logits, int64_t n, float cap, umb_stream_t st) {
  return call("umb_logit_softcap", logits, (long)n, cap, st);
}

// ---- the HIP runtime calls of model.hip (C linkage: the symbol names are all that has to match)
int hipEventRecord(void* event, void* stream) { call("hipEventRecord", event, stream); return hip_rc(); }
int hipStreamWaitEvent(void* stream, void* event, unsigned flags) { call("hipStreamWaitEvent", stream, event, (int)flags); return hip_rc(); }
int hipMemcpyAsync(void* dst, const void* src, size_t bytes, int kind, void* stream) {
  call("hipMemcpyAsync", dst, src, (unsigned long)bytes, kind, stream);
  return hip_rc();
}
int hipStreamSynchronize(void* stream) { call("hipStreamSynchronize", stream); return hip_rc(); }
const char* hipGetErrorString(int e) { call("hipGetErrorString", e); return "stub error"; }
}  // extern "C"

static int allreduce_hook(void* ctx, float* buf, int64_t count, umb_stream_t st) {
  call("allreduce_hook", ctx, buf, (long)count, st);
  return g_hook_rc;
}

// ------------------------------------------------------------------ the fixture a case edits
enum Entry { FWD, TP, OFF, G2, G2OFF, Q3, Q3OFF };
static const char* const kEntry[] = {"umb_model_forward", "umb_model_forward_tp", "umb_model_forward_offload",
                                     "umb_model_forward_gemma2", "umb_model_forward_gemma2_offload", "umb_model_forward_qwen3",
                                     "umb_model_forward_qwen3_offload"};
enum { LMAXL = 4 };                // layers a case may ask for
struct Fix {
  int entry = FWD;
  // model: qkv N = (Hq + 2 Hkv) D = 3072, o K = 2048, gate/up N = 16384
  int L = 1, H = 2048, I = 8192, Hq = 32, Hkv = 8, D = 64, V = 32000, Lmax = 4096, Tmax = 128, ssq_stride = 256;
  // step
  int T = 13, lb = 0, le = -1 /* L */, skip_embed = 0, head_from = 0 /* -1: T - 1, -2: T */;
  int tree = 0;                    // tree mode (tokens_all / n_ptr / depth) instead of explicit tokens
  // workspace
  int fused = 0, defer = 0, chain = 0;
  // linears
  int S_qkv = 2, S_o = 4, S_gu = 1, S_down = 4, S_row = 0, R = 1, R_gu = 1, tb = 0;
  int fmt = 0, fmt_layer = -1 /* every layer */, head_fmt = 0, head_S = 1;
  int bias = 0, bias_layer = -1;   // q/k/v bias on bias_layer (-1: every layer)
  int w_rows = 0, w_rows_upto = LMAXL, head_rows = 0;
  // tensor parallel
  int tp_null = 0, world = 2, rank = 0, hook = 1, peer = 0;
  long peer_max = 1 << 20, peer_cap = 1 << 20;
  // offload
  int off_null = 0, n_slabs = 2, pf = 0, forwards = 1;
  unsigned streamed = 0;           // bit l: layer l lives in a host slab
  // Gemma-2
  int g_null = 0, g_norms_null = 0, window = 0, parity = 0, no_pre_ff = -1, no_post_ff = -1;
  float final_softcap = 0.f;
  // Qwen3
  int q_null = 0, q_norms_null = 0, no_q_norm = -1, no_k_norm = -1;
  // stub rules
  int ll_wn = 4, gemv_ok = 1, chain_ok = 1, head_stream = 0, hook_rc = 0, hip_fail_at = 0;
};

// fake device addresses: small distinct integers, 16 apart, for everything model.hip only passes on; the buffers it offsets
// (the caches by layer, xn / hw / ssq by head_from) sit apart with room behind them
static uintptr_t g_next;
static void* fa() { g_next += 0x10; return (void*)g_next; }
template <class T> static T* fa() { return (T*)fa(); }
enum : uintptr_t { K_CACHE = 0x1000000, VT_CACHE = 0x2000000, XN = 0x3000000, HW = 0x3100000, SSQ = 0x3200000 };

// everything one case hands to model.hip; fake addresses are drawn in a fixed order, so they are the same in every case
struct World {
  UmbModel m = {};
  UmbLayer layers[LMAXL] = {};
  UmbWorkspace ws = {};
  UmbStep s = {};
  UmbTP tp = {};
  UmbTPPeer peer = {};
  UmbOffload off = {};
  void* host_slabs[LMAXL] = {};
  int32_t prefetched[UMB_MAX_SLABS];
  UmbGemma2 g = {};
  UmbGemma2Norms gn[LMAXL] = {};
  UmbQwen3 q = {};
  UmbQwen3Norms qn[LMAXL] = {};
  umb_stream_t st = nullptr;
};

static UmbLinear linear(const Fix& f, int N, int K, int S, int R, int fmt, bool streamed, bool rows, int idx) {
  UmbLinear l = {};
  void* w = fa(); void* meta = fa(); void* wr = fa();
  // a streamed layer's pointers are offsets into its slab, stored + 1
  l.w = streamed ? (void*)(uintptr_t)(1 + 0x1000 * idx) : w;
  l.meta = fmt == 0 ? nullptr : streamed ? (void*)(uintptr_t)(1 + 0x1000 * idx + 0x800) : meta;
  l.N = N; l.K = K; l.awq = fmt; l.R = R; l.S = S; l.tb = f.tb; l.S_row = f.S_row;
  l.w_rows = rows ? wr : nullptr;
  return l;
}

static void build(const Fix& f, World& w) {
  g_next = 0;
  UmbModel& m = w.m;
  m.dtype = 1; m.L = f.L; m.H = f.H; m.I = f.I; m.Hq = f.Hq; m.Hkv = f.Hkv; m.D = f.D; m.V = f.V; m.Lmax = f.Lmax;
  m.eps = 0.0625f; m.attn_scale = 0.125f;          // short exact values: they are printed on most lines
  m.embed = fa(); m.final_norm = fa(); m.rope_cos = fa(); m.rope_sin = fa();
  m.k_cache = (void*)K_CACHE; m.vt_cache = (void*)VT_CACHE;
  m.lm_head = linear(f, f.V, f.H, f.head_S, 1, f.head_fmt, false, f.head_rows, 0);
  m.layers = w.layers;
  for (int l = 0; l < LMAXL; ++l) {
    const bool str = (f.streamed >> l) & 1;
    const int fmt = (f.fmt_layer < 0 || f.fmt_layer == l) ? f.fmt : 0;
    const bool rows = f.w_rows && l < f.w_rows_upto;
    UmbLayer& y = w.layers[l];
    y.qkv = linear(f, (f.Hq + 2 * f.Hkv) * f.D, f.H, f.S_qkv, f.R, fmt, str, rows, 1);
    y.o = linear(f, f.H, f.Hq * f.D, f.S_o, f.R, fmt, str, rows, 2);
    y.gu = linear(f, 2 * f.I, f.H, f.S_gu, f.R_gu, fmt, str, rows, 3);
    y.down = linear(f, f.H, f.I, f.S_down, f.R, fmt, str, rows, 4);
    y.norm1 = fa(); y.norm2 = fa();
    void* b = fa();
    y.qkv_bias = (f.bias && (f.bias_layer < 0 || f.bias_layer == l)) ? b : nullptr;
    w.host_slabs[l] = str ? fa() : (fa(), nullptr);
    w.gn[l].pre_ff = fa(); w.gn[l].post_ff = fa();
    w.qn[l].q_norm = fa(); w.qn[l].k_norm = fa();
    if (f.no_pre_ff == l) w.gn[l].pre_ff = nullptr;
    if (f.no_post_ff == l) w.gn[l].post_ff = nullptr;
    if (f.no_q_norm == l) w.qn[l].q_norm = nullptr;
    if (f.no_k_norm == l) w.qn[l].k_norm = nullptr;
  }
  UmbWorkspace& ws = w.ws;
  ws.h = fa(); ws.xn = (void*)XN; ws.q = fa(); ws.attn = fa(); ws.act = fa(); ws.partial = fa<float>(); ws.attn_po = fa<float>();
  ws.attn_ml = fa<float>(); ws.pos = fa<int32_t>(); ws.slot = fa<int32_t>(); ws.prefix = fa<int32_t>(); ws.logits = fa<float>();
  ws.hw = (void*)HW; ws.ssq = (float*)SSQ; ws.counters = fa<uint32_t>(); ws.attn_counters = fa<uint32_t>();
  ws.Tmax = f.Tmax; ws.attn_chunk = 512; ws.attn_splits = 8; ws.ssq_stride = f.ssq_stride;
  ws.fused = f.fused; ws.defer_norm = f.defer;
  void* xchg = fa();
  ws.chain_xchg = f.chain ? xchg : nullptr;
  UmbStep& s = w.s;
  s.T = f.T; s.tree_off = f.tree ? 3 : 0;
  int32_t* tok = fa<int32_t>(); int32_t* pos = fa<int32_t>(); int32_t* slots = fa<int32_t>(); int32_t* all = fa<int32_t>();
  int32_t* nptr = fa<int32_t>(); int32_t* depth = fa<int32_t>();
  s.prefix_len = fa<int32_t>(); s.mask_bits = fa();
  if (f.tree) { s.tokens_all = all; s.n_ptr = nptr; s.depth = depth; } else { s.tokens = tok; s.positions = pos; s.slots = slots; }
  s.mask_words = 2; s.n_mask_keys = f.T;
  s.head_from = f.head_from == -1 ? f.T - 1 : f.head_from == -2 ? f.T : f.head_from;
  s.layer_begin = f.lb; s.layer_end = f.le == -1 ? f.L : f.le; s.skip_embed = f.skip_embed;
  w.st = (umb_stream_t)fa();
  // tensor parallel
  g_peer = &w.peer;
  w.peer.rank = f.rank; w.peer.world = f.world; w.peer.cap = f.peer_cap;
  w.tp.rank = f.rank; w.tp.world = f.world; w.tp.allreduce = f.hook ? allreduce_hook : nullptr; w.tp.ctx = fa();
  w.tp.peer = f.peer ? &w.peer : nullptr; w.tp.peer_max_floats = f.peer_max;
  // offload
  w.off.host_slabs = w.host_slabs; w.off.slab_bytes = 0x123400; w.off.copy_stream = (umb_stream_t)fa();
  for (int i = 0; i < UMB_MAX_SLABS; ++i) { w.off.dev_slab[i] = fa(); w.off.ev_copied[i] = fa(); w.off.ev_free[i] = fa(); }
  for (int i = 0; i < UMB_MAX_SLABS; ++i) w.prefetched[i] = -1;
  w.off.prefetched = f.pf ? w.prefetched : nullptr; w.off.n_slabs = f.n_slabs;
  // Gemma-2 / Qwen3
  w.g.attn_softcap = 50.f; w.g.final_softcap = f.final_softcap; w.g.embed_scale = 45.25f; w.g.window = f.window;
  w.g.slide_parity = f.parity; w.g.norms = f.g_norms_null ? nullptr : w.gn;
  w.q.qk_eps = 0.03125f; w.q.norms = f.q_norms_null ? nullptr : w.qn;
  g_ll_wn = f.ll_wn; g_gemv_ok = f.gemv_ok; g_chain_ok = f.chain_ok; g_head_stream = f.head_stream; g_hook_rc = f.hook_rc;
  g_hip_fail_at = f.hip_fail_at;
}

static int forward(const Fix& f, World& w) {
  const UmbOffload* off = f.off_null ? nullptr : &w.off;
  switch (f.entry) {
    case FWD: return umb_model_forward(&w.m, &w.ws, &w.s, w.st);
    case TP: return umb_model_forward_tp(&w.m, &w.ws, &w.s, f.tp_null ? nullptr : &w.tp, w.st);
    case OFF: return umb_model_forward_offload(&w.m, &w.ws, &w.s, off, w.st);
    case G2: return umb_model_forward_gemma2(&w.m, &w.ws, &w.s, f.g_null ? nullptr : &w.g, w.st);
    case G2OFF: return umb_model_forward_gemma2_offload(&w.m, &w.ws, &w.s, f.g_null ? nullptr : &w.g, off, w.st);
    case Q3: return umb_model_forward_qwen3(&w.m, &w.ws, &w.s, f.q_null ? nullptr : &w.q, w.st);
    default: return umb_model_forward_qwen3_offload(&w.m, &w.ws, &w.s, f.q_null ? nullptr : &w.q, off, w.st);
  }
}

// ------------------------------------------------------------------ the cases
struct Group { const char* name; const char* var; const char* value; };
static const Group kGroups[] = {
    {"base", nullptr, nullptr},
    {"split_fm_off", "UMB_SPLIT_FM", "0"},
    {"ll_draft_wide", "UMB_LL_DRAFT_WIDE", "1"},
    {"ll_gu_ll", "UMB_LL_GU", "ll"},
    {"ll_gu_shared", "UMB_LL_GU", "shared"},
    {"ll_qkv_ll", "UMB_LL_QKV", "ll"},
    {"ll_qkv_split", "UMB_LL_QKV", "split"},
    {"ll_head_ll", "UMB_LL_HEAD", "ll"},
    {"debug_sync", "UMB_DEBUG_SYNC", "1"},
};
struct Case { const char* name; const char* group; void (*edit)(Fix&); };
#define ROW(name, group, ...) {name, group, [](Fix& f) { __VA_ARGS__; }}
// low-latency model (fused 2); DRAFT: its linears also carry row-major copies (the GEMV / chain role)
#define LLM f.fused = 2
#define DRAFT f.fused = 2, f.w_rows = 1
// ll q/k/v on the split kernel: (64 + 16) 64 / 16 = 320 row groups, WN = 1 -> 320 blocks; gate/up off the shared kernel: R 2
#define QKV_SPLIT f.Hq = 64, f.ll_wn = 1
#define GU_LL f.R_gu = 2
static const Case kCases[] = {
    // ---- split schedule: row counts on both sides of 16 (FM operands), 64 / 65 (deferral, wide split), with the norm deferred or not
    ROW("split_t1", "base", f.T = 1),
    ROW("split_t13", "base", f.T = 13, f.L = 2),
    ROW("split_t16", "base", f.T = 16, f.L = 2),
    ROW("split_t64", "base", f.T = 64),
    ROW("split_t65", "base", f.T = 65),
    ROW("split_t100", "base", f.T = 100),
    ROW("defer_t1", "base", f.T = 1, f.defer = 1),
    ROW("defer_t13", "base", f.T = 13, f.defer = 1),
    ROW("defer_t16", "base", f.T = 16, f.defer = 1, f.L = 2),
    ROW("defer_t64", "base", f.T = 64, f.defer = 1),
    ROW("defer_t65", "base", f.T = 65, f.defer = 1),
    ROW("defer_t100", "base", f.T = 100, f.defer = 1),
    // H = 1024: (H / 512) % 4 != 0, use_defer refuses
    ROW("defer_refused_h1024_t13", "base", f.T = 13, f.defer = 1, f.H = 1024),
    ROW("defer_refused_ssq_stride", "base", f.T = 13, f.defer = 1, f.ssq_stride = 16),
    ROW("split_fm_refused_tmax", "base", f.T = 40, f.Tmax = 48),
    ROW("split_bias_t13", "base", f.T = 13, f.bias = 1),
    ROW("split_tree_mode_t13", "base", f.T = 13, f.tree = 1),
    // (one layer unless the case is about the layer sequence -- next norms, FM hand-over, ranges, the ring: it keeps the trace small)
    // eff_s: the plan's S_row; the cap branch (H 4096: 64 blocks x cap 4 = 256) taken and not (H 2048: 32 blocks)
    ROW("split_srow_t13", "base", f.T = 13, f.S_row = 3),
    ROW("split_cap_taken_t13", "base", f.T = 13, f.H = 4096, f.S_o = 8, f.S_down = 8),
    ROW("split_cap_not_taken_t13", "base", f.T = 13, f.S_o = 8, f.S_down = 8),
    // format 2 (FP8) layers
    ROW("split_fp8_t13", "base", f.T = 13, f.fmt = 2),
    ROW("split_fp8_t100", "base", f.T = 100, f.fmt = 2, f.S_o = 8),
    ROW("defer_fp8_t13", "base", f.T = 13, f.defer = 1, f.fmt = 2),
    ROW("split_awq_t13", "base", f.T = 13, f.fmt = 1),
    // layer ranges, head rows
    ROW("split_range_0_1", "base", f.L = 3, f.le = 1),
    ROW("split_range_1_L_skip_embed", "base", f.L = 3, f.lb = 1, f.skip_embed = 1),
    ROW("defer_range_1_L_skip_embed", "base", f.L = 3, f.lb = 1, f.skip_embed = 1, f.defer = 1),
    ROW("split_head_last", "base", f.head_from = -1),
    ROW("split_head_none", "base", f.head_from = -2),
    ROW("defer_head_last_t32", "base", f.T = 32, f.defer = 1, f.head_from = -1),
    ROW("defer_head_none", "base", f.defer = 1, f.head_from = -2),
    ROW("split_t16_fm_off", "split_fm_off", f.T = 16),
    ROW("defer_t64_fm_off", "split_fm_off", f.T = 64, f.defer = 1),
    ROW("q3_defer_t32_fm_off", "split_fm_off", f.entry = Q3, f.T = 32, f.defer = 1),
    // ---- fused schedule
    ROW("fused_t13", "base", f.fused = 1, f.L = 2),
    ROW("fused_t100_range_0_1", "base", f.fused = 1, f.T = 100, f.le = 1, f.L = 2),
    ROW("fused_bias_refused", "base", f.fused = 1, f.bias = 1),
    // ---- low-latency schedule, no row-major copies
    ROW("ll_t1", "base", LLM, f.T = 1),
    ROW("ll_t8", "base", LLM, f.T = 8, f.L = 2),
    ROW("ll_t16", "base", LLM, f.T = 16),
    ROW("ll_t64", "base", LLM, f.T = 64),
    ROW("ll_t65_leaves_for_split", "base", LLM, f.T = 65, f.defer = 1),
    ROW("ll_qkv_split_t8", "base", LLM, f.T = 8, QKV_SPLIT),
    ROW("ll_qkv_split_bias_t33", "base", LLM, f.T = 33, QKV_SPLIT, f.bias = 1),
    ROW("ll_gu_ll_t8", "base", LLM, f.T = 8, GU_LL),
    ROW("ll_gu_ssq_stride_odd", "base", LLM, f.T = 8, f.ssq_stride = 130),
    ROW("ll_bias_t8", "base", LLM, f.T = 8, f.bias = 1),
    ROW("ll_groups_exceed_stride", "base", LLM, f.T = 8, f.ssq_stride = 64),
    ROW("ll_range_0_1", "base", LLM, f.T = 8, f.L = 3, f.le = 1),
    ROW("ll_range_1_L_skip_embed", "base", LLM, f.T = 8, f.L = 3, f.lb = 1, f.skip_embed = 1),
    ROW("ll_head_shared_t16", "base", LLM, f.T = 16),
    ROW("ll_head_whole_k_head_last", "base", LLM, f.T = 16, f.head_from = -1),
    ROW("ll_head_whole_k_awq", "base", LLM, f.T = 16, f.head_fmt = 1),
    ROW("ll_head_stream_t6", "base", LLM, f.T = 6, f.head_rows = 1, f.head_stream = 1),
    ROW("ll_head_stream_not_ok_t6", "base", LLM, f.T = 6, f.head_rows = 1),
    ROW("ll_head_none", "base", LLM, f.T = 8, f.head_from = -2),
    ROW("ll_draft_t16_leaves_for_split", "base", DRAFT, f.T = 16, f.defer = 1),
    ROW("ll_draft_t8_stays", "base", DRAFT, f.T = 8, f.gemv_ok = 0),
    ROW("ll_draft_t16_kept", "ll_draft_wide", DRAFT, f.T = 16, f.defer = 1),
    ROW("ll_t8_gu_env_ll", "ll_gu_ll", LLM, f.T = 8),
    ROW("ll_t8_gu_env_shared", "ll_gu_shared", LLM, f.T = 8, GU_LL),
    ROW("ll_t8_qkv_env_ll", "ll_qkv_ll", LLM, f.T = 8, QKV_SPLIT),
    ROW("ll_t8_qkv_env_split", "ll_qkv_split", LLM, f.T = 8),
    ROW("ll_t16_head_env_ll", "ll_head_ll", LLM, f.T = 16),
    ROW("ll_t6_head_env_ll_stream", "ll_head_ll", LLM, f.T = 6, f.head_rows = 1, f.head_stream = 1),
    // ---- GEMV and chain
    ROW("gv_t1", "base", DRAFT, f.T = 1),
    ROW("gv_t4", "base", DRAFT, f.T = 4, f.L = 2),
    ROW("gv_t4_bias", "base", DRAFT, f.T = 4, f.bias = 1),
    ROW("gv_t5_is_ll", "base", DRAFT, f.T = 5),
    ROW("gv_not_ok_is_ll", "base", DRAFT, f.T = 2, f.gemv_ok = 0),
    ROW("gv_layer1_without_rows_is_ll", "base", DRAFT, f.T = 2, f.w_rows_upto = 1, f.L = 2),
    ROW("gv_groups_exceed_stride_is_ll", "base", DRAFT, f.T = 2, f.ssq_stride = 12),
    ROW("gv_head_stream", "base", DRAFT, f.T = 2, f.head_rows = 1, f.head_stream = 1),
    ROW("gv_head_stream_head_last", "base", DRAFT, f.T = 4, f.head_rows = 1, f.head_stream = 1, f.head_from = -1),
    ROW("gv_head_none", "base", DRAFT, f.T = 4, f.head_from = -2),
    ROW("gv_range_0_1", "base", DRAFT, f.T = 2, f.L = 3, f.le = 1),
    ROW("gv_range_1_L_skip_embed", "base", DRAFT, f.T = 2, f.L = 3, f.lb = 1, f.skip_embed = 1),
    ROW("chain_t1", "base", DRAFT, f.T = 1, f.chain = 1, f.L = 2),
    ROW("chain_t3_l3", "base", DRAFT, f.T = 3, f.chain = 1, f.L = 3),
    ROW("chain_t3_head_stream", "base", DRAFT, f.T = 3, f.chain = 1, f.head_rows = 1, f.head_stream = 1),
    ROW("chain_t4_not_ok_is_gv", "base", DRAFT, f.T = 4, f.chain = 1),
    ROW("chain_off_by_rule", "base", DRAFT, f.T = 2, f.chain = 1, f.chain_ok = 0),
    ROW("chain_stopped_by_bias", "base", DRAFT, f.T = 2, f.chain = 1, f.bias = 1, f.bias_layer = 1, f.L = 2),
    ROW("chain_stopped_by_ssq_stride", "base", DRAFT, f.T = 2, f.chain = 1, f.ssq_stride = 128),
    ROW("chain_range_0_1", "base", DRAFT, f.T = 2, f.chain = 1, f.L = 3, f.le = 1),
    ROW("chain_range_1_L", "base", DRAFT, f.T = 2, f.chain = 1, f.L = 3, f.lb = 1, f.skip_embed = 1),
    ROW("chain_xchg_on_ll_t8", "base", DRAFT, f.T = 8, f.chain = 1),
    // ---- tensor parallel
    ROW("tp_hook_t13", "base", f.entry = TP, f.L = 2),
    ROW("tp_hook_s1_no_sum", "base", f.entry = TP, f.S_o = 1, f.S_down = 1),
    ROW("tp_hook_fails", "base", f.entry = TP, f.hook_rc = 7),
    ROW("tp_peer_t13", "base", f.entry = TP, f.peer = 1, f.L = 2),
    ROW("tp_peer_range_0_1", "base", f.entry = TP, f.peer = 1, f.L = 3, f.le = 1),
    ROW("tp_peer_only_no_hook", "base", f.entry = TP, f.peer = 1, f.hook = 0),
    ROW("tp_peer_tile_too_large_takes_hook", "base", f.entry = TP, f.peer = 1, f.T = 100, f.peer_max = 100000),
    ROW("tp_peer_tile_too_large_no_hook_refused", "base", f.entry = TP, f.peer = 1, f.hook = 0, f.T = 100, f.peer_max = 100000),
    ROW("tp_fused1_refused", "base", f.entry = TP, f.fused = 1),
    ROW("tp_fused2_refused", "base", f.entry = TP, f.fused = 2, f.T = 8),
    ROW("tp_world1_is_plain", "base", f.entry = TP, f.world = 1, f.defer = 1),
    ROW("tp_world0_refused", "base", f.entry = TP, f.world = 0),
    ROW("tp_rank_negative_refused", "base", f.entry = TP, f.rank = -1),
    ROW("tp_rank_eq_world_refused", "base", f.entry = TP, f.rank = 2),
    ROW("tp_head_last_skip_embed", "base", f.entry = TP, f.L = 3, f.lb = 1, f.skip_embed = 1, f.head_from = -1),
    // ---- offload
    ROW("off_2slabs_mixed", "base", f.entry = OFF, f.L = 3, f.streamed = 0x5, f.fmt = 1),
    ROW("off_2slabs_all_streamed", "base", f.entry = OFF, f.L = 3, f.streamed = 0x7, f.fmt = 1, LLM, f.T = 8),
    ROW("off_none_streamed_pf", "base", f.entry = OFF, f.pf = 1),
    ROW("off_2slabs_pf_two_forwards_fits", "base", f.entry = OFF, LLM, f.T = 8, f.L = 3, f.streamed = 0x6, f.pf = 1, f.forwards = 2),
    ROW("off_2slabs_pf_two_forwards_exceeds", "base", f.entry = OFF, f.L = 3, f.streamed = 0x7, f.pf = 1, f.forwards = 2, LLM, f.T = 32),
    ROW("off_8slabs_pf_two_forwards", "base", f.entry = OFF, f.L = 3, f.streamed = 0x7, f.n_slabs = 8, f.pf = 1, f.forwards = 2,
        f.defer = 1),
    ROW("off_3slabs_pf_range_1_3", "base", f.entry = OFF, LLM, f.T = 8, f.L = 4, f.streamed = 0xf, f.n_slabs = 3, f.pf = 1, f.forwards = 2, f.lb = 1,
        f.le = 3, f.skip_embed = 1),
    ROW("off_defer_t13", "base", f.entry = OFF, f.streamed = 2, f.defer = 1, f.L = 2),
    ROW("off_fused_t13", "base", f.entry = OFF, f.streamed = 1, f.fused = 1),
    ROW("off_t100_head_last", "base", f.entry = OFF, f.streamed = 3, f.T = 100, f.head_from = -1, f.L = 2),
    ROW("off_ll_t2_stays_ll", "base", f.entry = OFF, DRAFT, f.T = 2, f.streamed = 2, f.chain = 1, f.L = 2),
    ROW("off_1slab_refused", "base", f.entry = OFF, f.streamed = 3, f.n_slabs = 1, f.L = 2),
    ROW("off_9slabs_refused", "base", f.entry = OFF, f.streamed = 3, f.n_slabs = 9, f.L = 2),
    ROW("off_copy_fails", "base", f.entry = OFF, f.streamed = 3, f.hip_fail_at = 4, f.L = 2),
    ROW("off_wait_fails", "base", f.entry = OFF, f.streamed = 3, f.hip_fail_at = 9, f.L = 2),
    // ---- Gemma-2
    ROW("g2_t13", "base", f.entry = G2, f.D = 128, f.Hq = 16),
    ROW("g2_t100_window_even", "base", f.entry = G2, f.T = 100, f.window = 1024, f.parity = 0, f.L = 2),
    ROW("g2_window_odd_softcap", "base", f.entry = G2, f.window = 1024, f.parity = 1, f.final_softcap = 30.f, f.L = 2),
    ROW("g2_head_none_softcap", "base", f.entry = G2, f.final_softcap = 30.f, f.head_from = -2),
    ROW("g2_head_last_softcap", "base", f.entry = G2, f.final_softcap = 30.f, f.head_from = -1),
    ROW("g2_off", "base", f.entry = G2OFF, f.L = 2, f.streamed = 2, f.window = 512, f.final_softcap = 30.f, f.pf = 1, f.forwards = 2),
    ROW("g2_null_refused", "base", f.entry = G2, f.g_null = 1),
    ROW("g2_norms_null_refused", "base", f.entry = G2, f.g_norms_null = 1),
    ROW("g2_fused_refused", "base", f.entry = G2, f.fused = 2),
    ROW("g2_range_begin_refused", "base", f.entry = G2, f.lb = 1, f.L = 2),
    ROW("g2_range_end_refused", "base", f.entry = G2, f.le = 1, f.L = 2),
    ROW("g2_skip_embed_refused", "base", f.entry = G2, f.skip_embed = 1),
    ROW("g2_window_negative_refused", "base", f.entry = G2, f.window = -1),
    ROW("g2_parity_refused", "base", f.entry = G2, f.parity = 2),
    ROW("g2_off_null_g_refused", "base", f.entry = G2OFF, f.g_null = 1),
    ROW("g2_missing_pre_ff", "base", f.entry = G2, f.no_pre_ff = 1, f.L = 2),
    ROW("g2_missing_post_ff", "base", f.entry = G2, f.no_post_ff = 0),
    ROW("g2_bias_refused_in_layer", "base", f.entry = G2, f.bias = 1, f.bias_layer = 1, f.L = 2),
    ROW("g2_off_missing_pre_ff", "base", f.entry = G2OFF, f.streamed = 3, f.no_pre_ff = 1, f.L = 2),
    // ---- Qwen3
    ROW("q3_t13", "base", f.entry = Q3),
    ROW("q3_fm_t32", "base", f.entry = Q3, f.T = 32, f.L = 2),
    ROW("q3_defer_t13", "base", f.entry = Q3, f.defer = 1, f.head_from = -1, f.L = 2),
    ROW("q3_defer_fm_t32", "base", f.entry = Q3, f.T = 32, f.defer = 1, f.L = 3),
    ROW("q3_off_t13", "base", f.entry = Q3OFF, f.streamed = 2, f.pf = 1, f.forwards = 2, f.L = 2),
    ROW("q3_off_defer_fm_t32", "base", f.entry = Q3OFF, f.T = 32, f.defer = 1, f.streamed = 1),
    ROW("q3_null_refused", "base", f.entry = Q3, f.q_null = 1),
    ROW("q3_norms_null_refused", "base", f.entry = Q3, f.q_norms_null = 1),
    ROW("q3_missing_q_norm_refused", "base", f.entry = Q3, f.no_q_norm = 1, f.L = 2),
    ROW("q3_missing_k_norm_refused", "base", f.entry = Q3, f.no_k_norm = 0),
    ROW("q3_fused_refused", "base", f.entry = Q3, f.fused = 2),
    ROW("q3_range_begin_refused", "base", f.entry = Q3, f.lb = 1, f.L = 2),
    ROW("q3_range_end_refused", "base", f.entry = Q3, f.L = 3, f.le = 2),
    ROW("q3_skip_embed_refused", "base", f.entry = Q3, f.skip_embed = 1),
    ROW("q3_d512_refused", "base", f.entry = Q3, f.D = 512),
    ROW("q3_off_null_refused", "base", f.entry = Q3OFF, f.off_null = 1),
    ROW("q3_off_1slab_refused", "base", f.entry = Q3OFF, f.n_slabs = 1),
    // ---- refusals common to the entry points
    ROW("fwd_lb_negative", "base", f.lb = -1),
    ROW("fwd_le_beyond_L", "base", f.le = 3),
    ROW("fwd_lb_eq_le", "base", f.lb = 1, f.le = 1, f.L = 2),
    ROW("tp_lb_negative", "base", f.entry = TP, f.lb = -1),
    ROW("tp_le_beyond_L", "base", f.entry = TP, f.le = 3),
    ROW("tp_lb_gt_le", "base", f.entry = TP, f.lb = 2, f.le = 1, f.L = 2),
    ROW("off_lb_negative", "base", f.entry = OFF, f.lb = -1),
    ROW("off_le_beyond_L", "base", f.entry = OFF, f.le = 3),
    ROW("off_lb_eq_le", "base", f.entry = OFF, f.lb = 1, f.le = 1, f.L = 2),
    ROW("g2_off_1slab_refused", "base", f.entry = G2OFF, f.n_slabs = 1),
    ROW("split_t0", "base", f.T = 0),
    ROW("split_t_beyond_tmax", "base", f.T = 129),
    ROW("defer_t0", "base", f.T = 0, f.defer = 1),
    ROW("fused_t_beyond_tmax", "base", f.fused = 1, f.T = 129),
    ROW("ll_t0", "base", LLM, f.T = 0),
    ROW("ll_t_beyond_tmax", "base", LLM, f.T = 33, f.Tmax = 32),
    ROW("gv_t0", "base", DRAFT, f.T = 0),
    ROW("gv_t_beyond_tmax", "base", DRAFT, f.T = 3, f.Tmax = 2),
    ROW("chain_t_beyond_tmax", "base", DRAFT, f.T = 3, f.Tmax = 2, f.chain = 1),
    ROW("tp_t0", "base", f.entry = TP, f.T = 0),
    ROW("off_t_beyond_tmax", "base", f.entry = OFF, f.streamed = 3, f.T = 129, f.L = 2),
    ROW("g2_t0", "base", f.entry = G2, f.T = 0),
    ROW("q3_t_beyond_tmax", "base", f.entry = Q3, f.T = 129),
    ROW("split_gu_s2", "base", f.S_gu = 2),
    ROW("defer_gu_s2", "base", f.S_gu = 2, f.defer = 1),
    ROW("fused_gu_s2", "base", f.S_gu = 2, f.fused = 1),
    ROW("tp_gu_s2", "base", f.entry = TP, f.S_gu = 2),
    ROW("off_gu_s2", "base", f.entry = OFF, f.S_gu = 2, f.streamed = 3, f.L = 2),
    ROW("q3_gu_s2", "base", f.entry = Q3, f.S_gu = 2, f.defer = 1),
    ROW("fp8_head_refused", "base", f.head_fmt = 2),
    ROW("fp8_head_tp_refused", "base", f.entry = TP, f.head_fmt = 2),
    ROW("fp8_head_off_refused", "base", f.entry = OFF, f.head_fmt = 2),
    ROW("fp8_head_g2_refused", "base", f.entry = G2, f.head_fmt = 2),
    ROW("fp8_head_q3_refused", "base", f.entry = Q3, f.head_fmt = 2),
    ROW("fp8_fused1_refused", "base", f.fmt = 2, f.fused = 1),
    ROW("fp8_fused2_refused", "base", f.fmt = 2, f.fused = 2, f.T = 8),
    ROW("fp8_fused2_t100_refused", "base", f.fmt = 2, f.fmt_layer = 1, f.fused = 2, f.T = 100, f.L = 2),
    ROW("fp8_chain_xchg_refused", "base", f.fmt = 2, f.chain = 1),
    ROW("fp8_w_rows_refused", "base", f.fmt = 2, f.w_rows = 1),
    ROW("fp8_outside_range_runs", "base", f.fmt = 2, f.fmt_layer = 2, f.L = 3, f.le = 2, f.fused = 1),
    ROW("fp8_tp_refused", "base", f.entry = TP, f.fmt = 2),
    ROW("fp8_tp_world1_runs", "base", f.entry = TP, f.fmt = 2, f.world = 1),
    ROW("fp8_off_refused", "base", f.entry = OFF, f.fmt = 2, f.fmt_layer = 1, f.L = 2),
    ROW("fp8_g2_refused", "base", f.entry = G2, f.fmt = 2, f.fmt_layer = 0),
    ROW("fp8_g2_off_refused", "base", f.entry = G2OFF, f.fmt = 2),
    ROW("fp8_q3_off_refused", "base", f.entry = Q3OFF, f.fmt = 2),
    ROW("fp8_q3_w_rows_refused", "base", f.entry = Q3, f.fmt = 2, f.w_rows = 1),
    // ---- UMB_DEBUG_SYNC=1: a synchronise behind every launch; the second case lets the third one fail
    ROW("sync_split_t13", "debug_sync", f.T = 13),
    ROW("sync_fails_at_third_launch", "debug_sync", f.T = 13, f.hip_fail_at = 3),
    ROW("sync_off_defer_t13", "debug_sync", f.entry = OFF, f.streamed = 2, f.defer = 1, f.L = 2),
    // the other schedules, so that where their synchronises fall is pinned too.  Gemma-2 and Qwen3 through their offload entry
    // points only: the model.hip the golden file was recorded from did not synchronise behind the head of a resident Gemma-2 /
    // Qwen3 forward, as every other entry point did; the shared layer loop does
    ROW("sync_ll_t8", "debug_sync", LLM, f.T = 8),
    ROW("sync_chain_t2", "debug_sync", DRAFT, f.T = 2, f.chain = 1, f.L = 2),
    ROW("sync_chain_range_0_1", "debug_sync", DRAFT, f.T = 2, f.chain = 1, f.le = 1, f.L = 2),
    ROW("sync_gv_range_0_1_head_stream", "debug_sync", DRAFT, f.T = 2, f.le = 1, f.L = 2),
    ROW("sync_tp_peer", "debug_sync", f.entry = TP, f.peer = 1),
    ROW("sync_g2_off", "debug_sync", f.entry = G2OFF, f.streamed = 1, f.final_softcap = 30.f),
};

static void run_case(const Case& c, int forwards_override) {
  Fix f;
  c.edit(f);
  World w;
  build(f, w);
  g_nasked = 0;
  if (!g_quiet) printf("== case %s entry=%s\n", c.name, kEntry[f.entry]);
  const int n = forwards_override > 0 ? forwards_override : f.forwards;
  for (int i = 0; i < n; ++i) {
    const int rc = forward(f, w);
    if (g_quiet) continue;
    printf("rc %d\n", rc);
    if (f.pf) {
      printf("prefetched");
      for (int k = 0; k < UMB_MAX_SLABS; ++k) printf(" %d", w.prefetched[k]);
      printf("\n");
    }
  }
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--groups")) {
    for (const Group& g : kGroups) printf("%s\n", g.name);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "--time")) {
    g_quiet = true;
    for (const Case& c : kCases) {
      if (strcmp(c.name, argv[2])) continue;
      for (const Group& g : kGroups)
        if (!strcmp(g.name, c.group) && g.var) setenv(g.var, g.value, 1);
      const int n = atoi(argv[3]);
      run_case(c, n / 10 + 1);                         // warm-up
      const auto t0 = std::chrono::steady_clock::now();
      run_case(c, n);
      const auto t1 = std::chrono::steady_clock::now();
      printf("%s %.1f ns/forward\n", c.name, std::chrono::duration<double, std::nano>(t1 - t0).count() / n);
      return 0;
    }
    fprintf(stderr, "no case %s\n", argv[2]);
    return 2;
  }
  if (argc != 2) { fprintf(stderr, "usage: model_trace --groups | GROUP | --time CASE N\n"); return 2; }
  for (const Group& g : kGroups) {
    if (strcmp(g.name, argv[1])) continue;
    for (const Group& o : kGroups)
      if (o.var) unsetenv(o.var);
    if (g.var) setenv(g.var, g.value, 1);
    printf("== group %s %s=%s\n", g.name, g.var ? g.var : "-", g.var ? g.value : "-");
    printf("umb_version %s\n", umb_version());
    for (const Case& c : kCases)
      if (!strcmp(c.group, g.name)) run_case(c, 0);
    return 0;
  }
  fprintf(stderr, "no group %s\n", argv[1]);
  return 2;
}
