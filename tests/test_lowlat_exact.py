"""Exact tests of the low-latency GEMM (csrc/lowlat.hip: ll_gemm_kernel) and the row-streaming GEMV (csrc/gemv.hip: gv_kernel):
every plan variable and every epilogue, whole buffers, bit for bit.  The persistent chain (chain.hip) is tested as "the same
bits as the GEMV launches", so the GEMV launches pinned here anchor the whole draft path.

Style and helpers are those of tests/test_gemm_exact.py (int_x, Lin, pack_rows_t, assert_same_bits, cached, the dev fixture; the
weights are packed by `pack` below, because mk_dense / mk_int4 know the interleave but not the RoPE row order; the bounds
functions acc_units / chain_bound).  No tolerance appears below: every comparison is assert_same_bits or torch.equal.

Operand regimes (every bound is evaluated on the CPU by test_exactness_bounds / test_token_rms_bounds / test_silu_bounds):

  integers   |x| <= 3; dense |W| <= 3, int4 codes under power-of-two scales (SCALE_EXPS).  The fp32 accumulator is exact in any
             order, for the MFMA chains, the LDS reduction over the WK slices and the v_dot2 chains + butterflies alike, so it
             equals the float64 matmul.  Dense K = 8192: at most 8192 * 9 = 73 728 units.
  regime A   ssq_in = NULL (the kernels set inv = 1.f literally).  Accumulators with MORE bits than the 16-bit formats hold
             (dense: x and W in 0 .. 3, sums of thousands; int4: 13 significant bits under the four scales), so every rounding
             of the epilogue contract is exercised.  The reference is torch float32 arithmetic on the CPU followed by
             .to(dtype): exact for a product of two 16-bit values; for a sum of two 16-bit values fp32-then-16-bit rounding
             equals direct rounding (24 >= 2 * 11 + 2); acc + bias is one IEEE fp32 add on both sides.
             test_rounding_discrimination_counts shows that the operands tell two roundings from one (residual add, RoPE).
  regime B   1/rms set: the producer's sums of squares are small integers c_g * 4^m_t in G groups (sum c_g = SSQ_DIM = 1024 =
             ssq_dim, eps = 0), m_t from RMS_M and different for neighbouring tokens: every partial sum in any order is exact
             and 1/rms = 2^-m_t.  The row stride is G + 5 and the columns behind the groups hold NaN: a read of them poisons the
             row.  Activations are sparse, so every expected output has few significant bits (asserted on the float64
             expectation in each test) and a last-bit error of the hardware rsqrt cannot move it.  Nothing bitwise is asserted
             about un-rounded fp32 output under 1/rms.
  SiLU       g / (1 + __expf(-g)) is g for every g >= 32 and 0 for g = 0 (test_silu_is_the_identity_from_32_up): gate weights
             are 0 or GATE = 64 and activations non-negative integers, so every scaled gate is 0 or >= 32 (1/rms >= 0.5) and
             the activation is rnd(rnd(g) * rnd(u)); operands are sparse enough that every gate * up is finite (asserted).
  ssq out    integer h (sparse rows, integer h0): every group's sum of squares is an integer below 2^24, compared group by
             group with a float64 sum of the squares of the reference h.

CPU part (no gpu mark): the bounds, the plan / pass tables, the SiLU identity, the rounding-discrimination counts, and the
reference functions of this module run as a MODEL with one seeded defect each on this module's operands: every defect must fail
assert_same_bits; which of them `max|a - b| / max|b| < 2e-2` (tests/test_lowlat.py, tests/test_gemv.py) lets through is
printed (run with -s) and reported, not asserted.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gemm_exact import (RMS_M, SCALE_EXPS, SPARSE_NNZ, WA, XA, OFFSETS, Lin, _gen, acc_units, assert_same_bits, cached,
                             chain_bound, dev, int_x, pack_rows_t)  # noqa: F401  (dev: the module-scoped device fixture)
from umbrella_amd.attn.cache import VT_PAD, k_offsets, vt_offsets

gpu = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [pytest.param(F16, id="f16"), pytest.param(BF16, id="bf16")]
EINVAL = -22
NAN = float("nan")
SENT = 7.0                                   # sentinel of the 16-bit buffers (a NaN pattern would do as well: bits are compared)

T_LL = (1, 15, 16, 17, 31, 32, 33, 48, 63, 64)
T_EPI = (1, 13, 17, 40, 64)
T_GV = (1, 2, 3, 4)
G_LL = (1, 3, 4, 31, 32, 33, 70)             # sums-of-squares groups against the 4 * WK read stride of ll_gemm_kernel
G_GV = (1, 64, 65, 255, 256)                 # ... against the four-values-per-lane read of gv_kernel
SSQ_DIM = 1024                               # sum of the group weights c_g = ssq_dim: s / dim = 4^m exactly
NNZ_I4 = 5                                   # regime B, int4 at scale 1.0: |acc| <= 5 * 3 * 15 = 225 < 2^8
NNZ_QKV_B = {"dense": 5, "int4": 2}          # regime B with an integer bias: |acc * inv + b| <= 2 * 90 + 3 (test_token_rms_bounds)
RMS_M_QKV = (-1, 0)                          # ... and 1/rms in {2, 1}, so that acc * inv + b stays an integer
GATE = 64.0                                  # the non-zero gate weight of the SiLU cases: GATE * 0.5 >= 32
NNZ_SILU_A, NNZ_SILU_B = 4, 3                # non-zeros per row of the SiLU cases (test_silu_bounds)
UP_SCALE = 2.0 ** -8                         # up weights are integers in -3 .. 3 times 2^-8: gate * up = a * b / 4
NNZ_SILU_WIDE = 512                          # fp16: rows wide enough that a * b has more than 11 significant bits, gate * up finite

# (N, K, WK, k-blocks per wave, idle row groups in the last block, blocks) of the dense plans; (N, K, R, WK, nk, idle, blocks) int4
DENSE_PLANS = [(16, 128, 1, 1, 7, 1), (64, 256, 2, 1, 0, 1), (208, 384, 1, 3, 3, 2), (208, 512, 4, 1, 1, 7), (320, 640, 1, 5, 4, 3),
               (1040, 768, 2, 3, 3, 17), (64, 1024, 8, 1, 0, 4), (512, 4096, 8, 4, 0, 32), (64, 6144, 8, 6, 0, 4),
               (64, 8192, 8, 8, 0, 4), (8256, 2048, 4, 4, 0, 258)]
INT4_PLANS = [(320, 384, 1, 1, 3, 4, 3), (64, 512, 1, 4, 1, 0, 2), (64, 4096, 1, 8, 4, 0, 4), (64, 8192, 1, 8, 8, 0, 4),
              (8192, 128, 2, 1, 1, 0, 32), (8192, 256, 2, 2, 1, 0, 64), (8256, 384, 2, 1, 3, 6, 33), (8192, 512, 2, 4, 1, 0, 128),
              (8192, 2048, 2, 8, 2, 0, 256), (8192, 4096, 2, 8, 4, 0, 256),
              (64, 2048, 1, 8, 2, 0, 4)]             # beyond the issue's list: the only way to <.., 1, TT 1, R 1, PF 2>
LL_CASES = [("dense", p[0], p[1]) for p in DENSE_PLANS] + [("int4", p[0], p[1]) for p in INT4_PLANS]
# epilogue plans: WK 1, 4 and 8 in both formats, the int4 one at N = 8192 with R = 2
EPI_CASES = [("dense", 320, 640, 1), ("dense", 512, 512, 4), ("dense", 512, 4096, 8),
             ("int4", 320, 384, 1), ("int4", 512, 512, 4), ("int4", 8192, 2048, 8)]
# (kind, Hq, Hkv, D, K, WK)
QKV_CASES = [("dense", 4, 2, 64, 4096, 8), ("dense", 3, 1, 32, 640, 1), ("dense", 2, 2, 128, 512, 4),
             ("int4", 4, 2, 64, 384, 1), ("int4", 2, 2, 128, 512, 4), ("int4", 48, 8, 128, 2048, 8)]
# GEMV launches: (N, K, passes)
GV_RESID = [(8, 2048, 1), (2048, 2048, 1), (2304, 2048, 2), (6144, 2048, 3), (16, 8192, 1), (2048, 8192, 1), (4096, 8192, 2),
            (8192, 8192, 4)]
GV_SILU = [(512, 2048, 1), (2048, 2048, 1), (4608, 2048, 2), (16384, 2048, 4)]
GV_QKV = [(3072, 32, 8, 64, 1), (6144, 32, 8, 128, 2), (512, 4, 2, 64, 1)]            # (N, Hq, Hkv, D, passes), K = 2048
# every (K, form) the GPU tests below use
USED_SHAPES = sorted({(K, kind) for kind, _, K in LL_CASES} | {(K, kind) for kind, _, K, _ in EPI_CASES}
                     | {(c[4], c[0]) for c in QKV_CASES} | {(2048, "dense"), (8192, "dense")})


def tt_of(T):
    """token tiles of the FM layout (umb_ll_token_tiles): 1, 2 or 4"""
    t = (T + 15) // 16
    return 4 if t == 3 else t


def ll_pf(T, awq, nk):
    """ring depth by the rule of ll_launch: the deepest of {4, 2, 1} that divides nk and fits the variant"""
    TT = tt_of(T)
    pfmax = 4 if TT == 1 else (1 if (TT == 4 and awq) else 2)
    return next(pf for pf in (4, 2, 1) if pf <= pfmax and nk % pf == 0)


def gv_geometry(N, K, epi):
    """(rows per wave RW, k-slices KS, row-group slots per pass, rows per block RB, passes) of a umb_gemv launch"""
    from umbrella_amd import _lib
    lib = _lib.load()
    RW = 4 if K == 8192 else (1 if epi == 4 else 2)
    KS = K // 2048
    # umb_gemv_groups answers for the residual epilogue (RW = 1 at K = 2048).  The pair epilogues (RW = 2, KS = 1) take the rows
    # per block from the same rule in steps of 2: rb = 2 r divides N exactly when r divides N / 2, and N / rb = (N / 2) / r, so
    # their block count is the library's answer for N / 2 rows.
    blocks = lib.umb_gemv_groups(4, N, K) if epi == 4 else lib.umb_gemv_groups(4, N // 2, K)
    RB = N // blocks
    nslot = 8 // KS
    return RW, KS, nslot, RB, -(-(RB // RW) // nslot)


# ------------------------------------------------------------------ bounds, plans (CPU)
@pytest.mark.parametrize("K,form", USED_SHAPES)
def test_exactness_bounds(K, form):
    assert acc_units(K, form) < 2 ** 24, (K, form, acc_units(K, form))
    if form == "dense":
        assert K * XA * WA <= 73728
        assert K >= 2048 or K * XA * W_WIDE < 2 ** 24                   # the wide weights of the small-K residual cases
        assert K * XA * GATE < 2 ** 24                                   # SiLU cases: gate weights 0 / 64, x in 0 .. 3
    else:
        for name, cs in OFFSETS.items():
            if name.startswith("lowlat"):
                for c in cs:
                    assert chain_bound(c) < 2 ** 24, (name, c)
        assert 15 * 2.0 ** max(SCALE_EXPS) < 65504 and 2.0 ** min(SCALE_EXPS) >= 2.0 ** -14
        assert K * XA * GATE < 2 ** 24                                   # int4 SiLU cases: gate = (8 q' - 0) * 8
    for dt in (F16, BF16):
        v = torch.arange(-256, 257, dtype=torch.float32)
        assert torch.equal(v.to(dt).float(), v)


def test_token_rms_bounds():
    """regime B: acc * 2^-m keeps acc's significand, so the expectation is a 16-bit value as soon as |acc| < 2^8 (bf16); the sums
    of squares and every partial sum of them are exact; integer h keeps every group's sum of squares below 2^24."""
    assert SPARSE_NNZ * XA * WA < 2 ** 8 and NNZ_I4 * XA * 15 < 2 ** 8
    for kind, nnz in NNZ_QKV_B.items():                                    # + integer bias, 1/rms in {2, 1}: an integer below 2^8
        assert all(2.0 ** -m == int(2.0 ** -m) for m in RMS_M_QKV)
        assert nnz * XA * (WA if kind == "dense" else 15) * max(2.0 ** -m for m in RMS_M_QKV) + 3 < 2 ** 8
    for G in set(G_LL) | set(G_GV) | {8}:
        for t in range(64):
            c = ssq_weights(G, t)
            assert len(c) == G and min(c) >= 1 and sum(c) == SSQ_DIM
            assert G == 1 or max(c) >= (SSQ_DIM - G) // 2 >= 256          # a heavy group carries a quarter of the sum at least
            for m in RMS_M:                                               # multiples of 4^-1 up to 4096: every partial sum is exact
                vals = np.array(c, dtype=np.float64) * 4.0 ** m
                assert np.array_equal(vals.astype(np.float32).astype(np.float64), vals) and vals.sum() * 4 < 2 ** 24
                assert float(np.float32(np.float32(vals.sum()) / np.float32(SSQ_DIM))) == 4.0 ** m
    for m in RMS_M:
        assert 256 * 2.0 ** -m < 65504 and 2.0 ** -m >= 2.0 ** -14
    # a last-bit error of the hardware rsqrt (2^-23 relative) against half an ulp of the 16-bit formats
    assert 4 * 2.0 ** -23 < 2.0 ** -12
    # sums of squares out: |h| <= 16 * 9 + 3 (dense) or 5 * 45 + 3 (int4), 32 columns per row group / at most 32 rows per block
    assert max(SPARSE_NNZ * XA * WA + 3, NNZ_I4 * XA * 15 + 3) ** 2 * 32 < 2 ** 24
    assert max(gv_geometry(N, K, 4)[3] for N, K, _ in GV_RESID) <= 32


def test_silu_bounds():
    """gates 0 or >= 32 after the smallest 1/rms; gate * up finite in fp16 on the sparse rows, and a value with at most 8
    significant bits in regime B (so bf16 holds it)"""
    assert GATE * min(2.0 ** -m for m in RMS_M) >= 32.0
    a_max = lambda nnz: nnz * XA                                          # gate = GATE * a, a = sum of x over the open gates
    u_max = lambda nnz: nnz * XA * WA
    assert GATE * a_max(NNZ_SILU_A) * u_max(NNZ_SILU_A) * UP_SCALE <= 65504
    assert 3 * UP_SCALE >= 2.0 ** -14 and 8192 * XA * WA < 2 ** 24        # ups are fp16 normals; up sums in units of 2^-8
    inv2 = max(2.0 ** -m for m in RMS_M) ** 2
    assert GATE * a_max(NNZ_SILU_B) * u_max(NNZ_SILU_B) * UP_SCALE * inv2 <= 65504
    assert a_max(NNZ_SILU_B) * u_max(NNZ_SILU_B) < 2 ** 8
    assert float(torch.tensor(GATE * 3 * 4096 * 9 * 4096).to(BF16)) < float("inf")      # bf16 dense rows: finite


def test_silu_is_the_identity_from_32_up():
    """g / (1 + exp(-g)) == g in fp32 for EVERY finite fp16 and bf16 value g >= 32 (1 + e == 1 for e <= 2^-25, exp(-32) is eleven
    orders below, whatever the last bits of the fast exponential), and 0 for g = 0"""
    one = np.float32(1.0)
    assert float(np.exp(-32.0)) * 1e6 < 2.0 ** -25 and one + np.float32(2.0 ** -25) == one
    for dt in (F16, BF16):
        bits = torch.arange(0, 0x7c00 if dt == F16 else 0x7f80, dtype=torch.int32).to(torch.int16)
        g = bits.view(dt).float().numpy()
        g = g[g >= 32.0]
        assert g.size > 1000
        with np.errstate(under="ignore"):
            e = np.exp(-g).astype(np.float32)
            assert np.array_equal(g / (one + e), g)
            assert np.array_equal(g / (one + e * np.float32(1.01)), g)
    assert np.float32(0.0) / (one + np.float32(np.exp(np.float32(-0.0)))) == 0.0


def _plan(N, K, awq):
    from umbrella_amd.models.llama import ll_plan
    return ll_plan(N, K, awq)


def test_plans_reach_every_variable():
    """the shapes of section 1 under the plan the library really takes: WK 1 / 2 / 4 / 8, ring depths 1 / 2 / 4 with and without
    the steady-state loop, the int4 metadata ring under PF = 4, R 1 / 2, idle row groups, a grid above 256 blocks"""
    seen_wk, seen_ring, seen_r, seen = set(), set(), set(), set()
    for N, K, WK, nk, idle, blocks in DENSE_PLANS:
        R, WN, wk, NW = _plan(N, K, False)
        groups = N // 16 // R
        assert (R, wk, K // 128 // wk, -(-groups // WN) * WN - groups, -(-groups // WN)) == (1, WK, nk, idle, blocks), (N, K)
        assert NW == 8 and WN * wk == 8
        seen_wk.add(wk)
        seen_r.add(R)
        seen |= {"idle"} if idle else set()
        seen |= {"grid>256"} if blocks > 256 else set()
        for T in T_LL:
            pf = ll_pf(T, False, nk)
            seen_ring.add((0, tt_of(T), pf, nk >= 2 * pf))
    for N, K, R, WK, nk, idle, blocks in INT4_PLANS:
        r, WN, wk, NW = _plan(N, K, True)
        groups = N // 16 // r
        assert (r, wk, K // 128 // wk, -(-groups // WN) * WN - groups, -(-groups // WN)) == (R, WK, nk, idle, blocks), (N, K)
        seen_wk.add(("int4", wk))
        seen_r.add(("int4", r))
        seen |= {"int4 idle R2"} if idle and r == 2 else set()
        for T in T_LL:
            pf = ll_pf(T, True, nk)
            seen_ring.add((1, tt_of(T), pf, nk >= 2 * pf))
    assert {1, 2, 4, 8} <= seen_wk and {("int4", w) for w in (1, 2, 4, 8)} <= seen_wk
    assert {1, ("int4", 1), ("int4", 2)} <= seen_r and {"idle", "grid>256", "int4 idle R2"} <= seen
    for pf in (1, 2, 4):                # int4 reaches all six; dense all but PF = 2 without the loop (no dense plan of the table has nk = 2)
        for steady in (False, True):
            assert any(r[0] == 1 and r[2] == pf and r[3] == steady for r in seen_ring), (pf, steady)
            assert (pf, steady) == (2, False) or any(r[0] == 0 and r[2] == pf and r[3] == steady for r in seen_ring), (pf, steady)
    # the table of the issue: PF 1 steady (nk 5), PF 4 at one token tile and PF 2 steady at two / four (nk 4), PF 2 steady at one
    # (nk 6), PF 4 steady (nk 8); TT = 4 with an empty fourth tile is T = 33 .. 48; int4 at TT = 4 always runs PF = 1
    assert ll_pf(16, False, 5) == 1 and ll_pf(16, False, 4) == 4 and ll_pf(32, False, 4) == 2 and ll_pf(64, False, 4) == 2
    assert ll_pf(16, False, 6) == 2 and ll_pf(16, False, 8) == 4 and ll_pf(48, True, 8) == 1 and ll_pf(16, True, 4) == 4
    assert tt_of(33) == 4 and tt_of(48) == 4 and tt_of(32) == 2
    for kind, N, K, WK in EPI_CASES:
        assert _plan(N, K, kind == "int4")[2] == WK, (kind, N, K)
    assert _plan(8192, 2048, True)[0] == 2
    for kind, Hq, Hkv, D, K, WK in QKV_CASES:
        assert _plan((Hq + 2 * Hkv) * D, K, kind == "int4")[2] == WK, (kind, Hq, Hkv, D, K)
    assert _plan(8192, 2048, True)[0] == 2 and (48 + 16) * 128 == 8192


def test_gemv_launch_shapes():
    """1, 2, 3 and 4 passes at both K; a single row per block with 7 idle waves; a second pass with one busy slot; 6 of 8 slots"""
    from umbrella_amd import _lib
    lib = _lib.load()
    for N, K, passes in GV_RESID:
        assert lib.umb_gemv_ok(4, N, K, 4) == 1
        assert gv_geometry(N, K, 4)[4] == passes, (N, K, gv_geometry(N, K, 4))
    assert gv_geometry(8, 2048, 4)[3] == 1 and gv_geometry(2304, 2048, 4)[3] == 9 and gv_geometry(16, 8192, 4)[3] == 8
    assert lib.umb_gemv_groups(4, 16, 8192) == 2 and lib.umb_gemv_groups(4, 8, 2048) == 8
    for N, K, passes in GV_SILU:
        assert lib.umb_gemv_ok(4, N, K, 2) == 1 and gv_geometry(N, K, 2)[4] == passes, (N, gv_geometry(N, K, 2))
    for N, Hq, Hkv, D, passes in GV_QKV:
        assert N == (Hq + 2 * Hkv) * D and lib.umb_gemv_ok(4, N, 2048, 3) == 1
        assert gv_geometry(N, 2048, 3)[4] == passes, (N, gv_geometry(N, 2048, 3))
    assert gv_geometry(3072, 2048, 3)[3] // 2 == 6 and gv_geometry(6144, 2048, 3)[3] // 2 == 12
    assert {p for _, K, p in GV_RESID if K == 2048} == {1, 2, 3} and {p for _, K, p in GV_RESID if K == 8192} == {1, 2, 4}


# ------------------------------------------------------------------ the reference: float32 torch on the CPU, one step per rounding
def rnd(v, dtype):
    return v.to(dtype).float()


def exact32(v64):
    """a float64 matmul of integer operands as fp32, asserted exact"""
    f = v64.float()
    assert torch.equal(f.double(), v64)
    return f


def ssq_weights(G, t=0):
    """integer group weights of token t, sum SSQ_DIM: 1 everywhere and the rest on two groups whose places move with the token
    (counted from the last group and from the first), so that a dropped group changes 1/rms by far more than a 16-bit ulp for
    some token of every launch -- a few-bit expectation would absorb the loss of a light group"""
    c = [1] * G
    rest = SSQ_DIM - G
    c[(G - 1 - 3 * t) % G] += rest // 2
    c[(7 * t) % G] += rest - rest // 2
    return c


def ssq_rows(T, G, ms=RMS_M):
    """(ssq [T, G + 5] fp32 on the CPU, 1/rms [T] float64): G valid groups c_g * 4^m_t, NaN behind them"""
    m = torch.tensor(ms, dtype=torch.float64)[torch.arange(T) % len(ms)]
    ssq = torch.full((T, G + 5), NAN, dtype=torch.float32)
    ssq[:, :G] = (torch.tensor([ssq_weights(G, t) for t in range(T)], dtype=torch.float64) * 4.0 ** m[:, None]).float()
    return ssq, 2.0 ** -m


def model_acc(x64, Wd, WK=1, defect=None):
    """x . W summed as WK interleaved k-slices (slice wk owns k-blocks wk, wk + WK, ..), float64 -> fp32"""
    KB = x64.shape[1] // 128
    out = torch.zeros(x64.shape[0], Wd.shape[1], dtype=torch.float64, device=x64.device)
    for wk in range(WK):
        if defect == "wk_sibling_partial_dropped" and wk == 1:
            continue
        for kb in range(wk, KB, WK):
            out += x64[:, kb * 128:(kb + 1) * 128] @ Wd[kb * 128:(kb + 1) * 128]
    return exact32(out)


def model_inv(ssq, G, defect=None):
    """1/rms per token from the first G columns of ssq (float64; exact powers of two on this module's operands)"""
    use = min(G, 64) if defect == "ssq_groups_beyond_64_ignored" else G
    inv = 1.0 / torch.sqrt(ssq[:, :use].double().sum(1) / SSQ_DIM)
    if defect == "inv_from_token_t_plus_1":
        inv = torch.roll(inv, -1)
    return inv


def model_logits(acc, T, dtype, inv=None, round_out=False, row_from=0, defect=None):
    """epi 0 on a NaN-filled [T, N] buffer: rows row_from .. T-1 land at 0 .."""
    out = torch.full((T, acc.shape[1]), NAN, dtype=torch.float32)
    v = acc[:T].double()
    if inv is not None:
        v = v * inv[:T, None]
    v = exact32(v) if inv is None else v.float()
    if round_out:
        v = rnd(v, dtype)
    rf = row_from + 1 if defect == "row_from_off_by_one" else row_from
    out[:T - rf] = v[rf:]
    return out


def model_silu(acc, dtype, inv=None, defect=None):
    """acc [T, 2 I] fp32 with (gate_m, up_m) in columns (2m, 2m + 1) -> act [T, I]; SiLU is the identity on the gate set"""
    v = acc if inv is None else (acc.double() * inv[:, None]).float()
    g, u = rnd(v[:, 0::2], dtype), rnd(v[:, 1::2], dtype)
    if defect == "gate_and_up_swapped_in_a_pair":
        g, u = u, g
    if defect is None:
        assert bool(((g == 0) | (g >= 32)).all()), "a scaled gate is neither 0 nor >= 32"
    act = (rnd(g / (1.0 + torch.exp(-g)), dtype) * u).to(dtype)          # the identity on the gate set; not on a swapped-in up
    assert defect or bool(torch.isfinite(act.float()).all()), "gate * up is not finite in the dtype"
    return act


def model_resid(acc, h0, nw, dtype, defect=None):
    """h = rnd(rnd(acc) + h0); hw = rnd(h * w_next)"""
    o = rnd(acc, dtype)
    h = rnd(acc + h0.float(), dtype) if defect == "one_rounding_in_the_residual_add" else rnd(o + h0.float(), dtype)
    src = h0.float() if defect == "hw_from_h_before_the_add" else h
    hw = None if nw is None else (src * nw.float()[None]).to(dtype)
    return h.to(dtype), hw


def group_ssq(h, cols):
    """per group of `cols` consecutive columns: float64 sum of squares as fp32, asserted exact (integers below 2^24)"""
    T, N = h.shape
    s = h.double().pow(2).view(T, N // cols, cols).sum(-1)
    assert float(s.max()) < 2 ** 24
    return exact32(s)


def model_qkv(acc, dtype, pos, cos, sin, Hq, Hkv, D, inv=None, bias=None, defect=None):
    """acc [T, N] fp32 in HF feature order -> q [T, Hq, D], k [T, Hkv, D], v [T, Hkv, D] in the model dtype"""
    T = acc.shape[0]
    v = acc if inv is None else (acc.double() * inv[:, None]).float()
    if bias is not None:
        v = v + bias.float()[None]                                          # one fp32 add, then one rounding
    y = rnd(v, dtype).view(T, Hq + 2 * Hkv, D)
    half = D // 2
    c, s = cos[pos.long()].float()[:, None, :], sin[pos.long()].float()[:, None, :]
    a, b = y[:, :Hq + Hkv, :half], y[:, :Hq + Hkv, half:]
    s_lo = -s[..., :half] if defect == "sign_of_sin_on_the_low_half" else s[..., :half]
    lo = rnd(rnd(a * c[..., :half], dtype) + rnd(-b * s_lo, dtype), dtype)
    hi = rnd(rnd(b * c[..., half:], dtype) + rnd(a * s[..., half:], dtype), dtype)
    rot = torch.cat([lo, hi], -1).to(dtype)
    return rot[:, :Hq].contiguous(), rot[:, Hq:].contiguous(), y[:, Hq + Hkv:].to(dtype).contiguous()


def rope_single_rounded(acc, dtype, pos, cos, sin, Hq, Hkv, D, bias=None):
    """the low halves with ONE rounding of a c - b s (float64 sum of two exact products)"""
    T = acc.shape[0]
    y = rnd(acc if bias is None else acc + bias.float()[None], dtype).view(T, Hq + 2 * Hkv, D).double()
    half = D // 2
    c, s = cos[pos.long()].double()[:, None, :half], sin[pos.long()].double()[:, None, :half]
    return (y[:, :Hq + Hkv, :half] * c - y[:, :Hq + Hkv, half:] * s).float().to(dtype)


def fm_index(T, F, TT):
    """element offsets of (t, f) in an FM buffer of TT token tiles (csrc/common.h fm_off) -> [T, F]"""
    t, f = torch.arange(T)[:, None], torch.arange(F)[None, :]
    return ((((f >> 5) * TT + (t >> 4)) * 64 + ((f >> 3) & 3) * 16 + (t & 15)) << 3) + (f & 7)


def fm_expected(rows, TT):
    """the whole FM buffer: sentinel everywhere (pad tokens of the last tile included) except rows [T, F] at their offsets"""
    T, F = rows.shape
    buf = torch.full((TT * 16 * F,), SENT, dtype=rows.dtype)
    buf[fm_index(T, F, TT).reshape(-1)] = rows.reshape(-1)
    return buf


def cache_expected(k, v, slot, Lmax, defect=None):
    """sentinel-filled raw K [Hkv, Lmax, D] and V^T [Hkv, D, Lmax + VT_PAD] storage with exactly the appended elements replaced"""
    T, Hkv, D = k.shape
    sl = slot.long()
    if defect == "slot_of_the_neighbouring_token":
        sl = torch.roll(sl, 1)
    kc = torch.full((Hkv, Lmax, D), SENT, dtype=k.dtype)
    vt = torch.full((Hkv, D, Lmax + VT_PAD), SENT, dtype=k.dtype)
    kc.view(Hkv, -1)[:, k_offsets(sl, D)] = k.permute(1, 0, 2)
    vt.view(Hkv, -1)[:, vt_offsets(sl, D)] = v.permute(1, 2, 0)
    return kc, vt


def pick_pos_slot(T, P, Lmax, seed):
    """pos includes 0 and the table's last row; slot includes 0, 31, 32, Lmax-1 and is a permutation across the 32-key tiles"""
    g = torch.Generator().manual_seed(seed)
    pos = torch.randint(0, P, (T,), generator=g, dtype=torch.int32)
    pos[0] = P - 1 if T % 2 else 0
    if T > 1:
        pos[-1] = 0 if T % 2 else P - 1
    special = [0, 31, 32, Lmax - 1]
    special = special[T % 4:] + special[:T % 4]
    rest = [s for s in torch.randperm(Lmax, generator=g).tolist() if s not in special]
    slot = torch.tensor((special + rest)[:T], dtype=torch.int32)
    return pos, slot[torch.randperm(T, generator=g)]


# ------------------------------------------------------------------ operands
W_WIDE = 15                                  # dense |W| of the regime A residual cases below K = 2048 (test_exactness_bounds)


def gen_w(kind, N, K, dev, seed, nonneg=False, s1=False, wmax=WA):
    """float64 weights and what packs them: dense W [N, K] integers; int4 (q, z, s) with Wd = (q - z) s [K, N]"""
    g = _gen(dev, seed)
    if kind == "dense":
        W = torch.randint(0 if nonneg else -wmax, wmax + 1, (N, K), device=dev, generator=g).double()
        return W, W.t().contiguous()
    q = torch.randint(0, 16, (K, N), device=dev, generator=g, dtype=torch.uint8)
    z = torch.randint(0, 16, (K // 128, N), device=dev, generator=g, dtype=torch.uint8)
    if s1:
        s = torch.ones(K // 128, N, device=dev).half()
    else:
        e = torch.randint(0, len(SCALE_EXPS), (K // 128, N), device=dev, generator=g)
        s = torch.tensor([2.0 ** v for v in SCALE_EXPS], device=dev)[e].half()
    Wd = (q.double() - z.double().repeat_interleave(128, 0)) * s.double().repeat_interleave(128, 0)
    return (q, z, s), Wd


def gen_silu_w(kind, I, K, dev, seed):
    """[gate; up] stack with gates 0 / GATE and ups in -3 .. 3; returns (pack source, Wd [K, 2 I] in HF column order)"""
    g = _gen(dev, seed)
    on = torch.randint(0, 2, (K, I), device=dev, generator=g)
    up = torch.randint(-3, 4, (K, I), device=dev, generator=g)
    Wd = torch.cat([on.double() * GATE, up.double() * UP_SCALE], 1)
    if kind == "dense":
        return Wd.t().contiguous(), Wd
    q = torch.cat([on * 8, up + 8], 1).to(torch.uint8)                    # gate = (8 q' - 0) * 8, up = (q - 8) * 2^-8
    z = torch.cat([torch.zeros(K // 128, I, device=dev), torch.full((K // 128, I), 8.0, device=dev)], 1).to(torch.uint8)
    s = torch.cat([torch.full((K // 128, I), GATE / 8, device=dev), torch.full((K // 128, I), UP_SCALE, device=dev)], 1).half()
    return (q, z, s), Wd


def pack(kind, src, Wd, dtype, mode=None):
    """PackedLinear of gen_w's output; mode None | "il" | (D, rope heads).  o.Wd [K, N] float64 stays in HF column order."""
    from umbrella_amd.models.llama import PackedLinear
    kw = {"interleave": True} if mode == "il" else ({"rope": mode} if mode else {})
    o = Lin()
    if kind == "dense":
        o.lin = PackedLinear.from_dense(src.to(dtype), **kw)
    else:
        q, z, s = src
        o.lin = PackedLinear.from_awq(pack_rows_t(q), pack_rows_t(z), s, **kw)
    o.Wd, o.N, o.K, o.awq = Wd, Wd.shape[1], Wd.shape[0], int(kind == "int4")
    return o


def ll_lin(kind, N, K, dtype, dev, s1=False, nonneg=False, wmax=WA):
    key = ("lle-lin", kind, N, K, dtype if kind == "dense" else None, s1, nonneg, wmax)
    return cached(key, lambda: pack(kind, *gen_w(kind, N, K, dev, 500 + N + K + s1, nonneg=nonneg, s1=s1, wmax=wmax), dtype))


def xs_for(K, dev, nnz=None, nonneg=False):
    x = cached(("lle-x", K, nnz), lambda: int_x(64, K, dev, 700 + K + (nnz or 0), nnz=nnz))
    return x.abs() if nonneg else x


def _fx(cls=None, **kw):
    """a filled UmbGemmLL (cls: another argument struct of _lib, e.g. UmbGemmFused); tensors are kept alive on the struct"""
    from umbrella_amd import _lib
    fx = (cls or _lib.UmbGemmLL)()
    keep = []
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            keep.append(v)
            v = v.data_ptr()
        elif v is None:
            v = 0
        setattr(fx, k, v)
    fx._keep = keep
    return fx


def rms_kw(ssq_dev, G):
    return dict(ssq_in=ssq_dev, ssq_groups=G, ssq_in_stride=ssq_dev.shape[1], ssq_dim=float(SSQ_DIM), eps=0.0)


def same(got, want, what):
    """whole buffers of any rank, bit for bit (assert_same_bits reports (split, row, column) of a 3-d view)"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dim() == 1:
        got, want = got[None, None], want[None, None]
    elif got.dim() == 2:
        got, want = got[None], want[None]
    elif got.dim() > 3:
        got, want = got.reshape(-1, *got.shape[-2:]), want.reshape(-1, *want.shape[-2:])
    assert_same_bits(got, want, what)


def sent(shape, dtype, dev):
    return torch.full(shape, SENT, dtype=dtype, device=dev)


# ------------------------------------------------------------------ 1. ll_gemm_kernel: every plan variable
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,N,K", LL_CASES)
def test_ll_logits_every_plan(dev, kind, N, K, dtype):
    """epi 0 under the library's own plan at every token-tile class: un-rounded and rounded against the float64 matmul (regime
    A), row_from on a NaN-filled buffer, and the rounded output under exact per-token 1/rms for every group count (regime B)"""
    awq = kind == "int4"
    R, WN, WK, NW = _plan(N, K, awq)
    o = ll_lin(kind, N, K, dtype, dev)
    ob = ll_lin(kind, N, K, dtype, dev, s1=True) if awq else o               # regime B, int4: all scales 1.0 (integers)
    xd, xs = xs_for(K, dev), xs_for(K, dev, nnz=NNZ_I4 if awq else SPARSE_NNZ)
    ref = cached(("lle-ref", kind, N, K), lambda: exact32(xd @ o.Wd).cpu())
    refs = cached(("lle-refs", kind, N, K), lambda: exact32(xs @ ob.Wd).cpu())
    n = 0
    for T in T_LL:
        x16, what = xd[:T].to(dtype), f"{kind} N={N} K={K} WK={WK} R={R} T={T} PF={ll_pf(T, awq, K // 128 // WK)}"
        same(o.lin.apply_ll(x16), model_logits(ref, T, dtype), what + " raw")
        same(o.lin.apply_ll(x16, round_out=True), model_logits(ref, T, dtype, round_out=True), what + " rounded")
        for rf in sorted({0, 1, 15, 16, T - 1} & set(range(T))):
            out = torch.full((T, N), NAN, dtype=torch.float32, device=dev)
            o.lin.apply_ll(x16, fx=_fx(row_from=rf), out=out)
            same(out, model_logits(ref, T, dtype, row_from=rf), what + f" row_from={rf}")
            n += 1
        xs16 = xs[:T].to(dtype)
        for G in G_LL:
            ssq, inv = ssq_rows(T, G)
            want64 = refs[:T].double() * inv[:, None]
            want = model_logits(refs, T, dtype, inv=model_inv(ssq, G), round_out=True)
            assert torch.equal(want.double(), want64), f"{what}: an expected value is not a {dtype} value"
            got = ob.lin.apply_ll(xs16, round_out=True, fx=_fx(**rms_kw(ssq.to(dev), G)))
            same(got, want, what + f" 1/rms G={G}")
            n += 1
    assert n >= len(T_LL) * (len(G_LL) + 1)


# ------------------------------------------------------------------ 2. ll_gemm_kernel: epilogues
def silu_variants(dtype):
    """(name, non-zeros per row, regime B).  The sparse variants have few-bit products (regime B needs that).  The roundings are
    exercised by dense rows in bf16 (gates, ups and products all beyond 8 bits; fp16 cannot hold those gates) and by rows of
    NNZ_SILU_WIDE non-zeros in fp16: a gate 64 a below 65504 is always an fp16 value, and so is an up b / 256 with b < 2^11, but
    the product a b / 4 has up to 17 significant bits and stays finite -- rnd(g * u) is a real rounding there."""
    v = [("A-sparse", NNZ_SILU_A, False), ("B-sparse", NNZ_SILU_B, True)]
    return v + ([("A-dense", None, False)] if dtype == BF16 else [("A-wide", NNZ_SILU_WIDE, False)])


def silu_rounds(acc, want, name):
    """the wide / dense variants must contain products that the dtype does not hold: the last rounding is then a real one"""
    if name in ("A-dense", "A-wide"):
        exact = acc[:, 0::2].double() * acc[:, 1::2].double()
        n = int((want.double() != exact).sum())
        assert n > 0, f"{name}: every gate * up is a {want.dtype} value, the rounding of the product is not exercised"


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,N,K,WK", EPI_CASES)
def test_ll_silu_epilogue_exact(dev, kind, N, K, WK, dtype):
    """epi 2: the whole FM activation buffer (pad tokens keep the sentinel), through fm_off and through umb_from_fm"""
    from umbrella_amd.models.llama import from_fm
    I = N // 2
    o = cached(("lle-silu", kind, N, K, dtype if kind == "dense" else None),
               lambda: pack(kind, *gen_silu_w(kind, I, K, dev, 800 + N + K), dtype, mode="il"))
    il = torch.stack([torch.arange(I), I + torch.arange(I)], 1).reshape(-1).to(dev)       # output column 2m / 2m+1 <- gate m / up m
    for name, nnz, regb in silu_variants(dtype):
        x = xs_for(K, dev, nnz=nnz and min(nnz, K), nonneg=True)
        acc = exact32(x @ o.Wd[:, il]).cpu()
        for T in T_EPI:
            what = f"SiLU {kind} N={N} K={K} WK={WK} T={T} {name}"
            kw, inv = {}, None
            if regb:
                ssq, _ = ssq_rows(T, 8)
                kw, inv = rms_kw(ssq.to(dev), 8), model_inv(ssq, 8)
            want = model_silu(acc[:T], dtype, inv=inv)
            silu_rounds(acc[:T], want, name)
            if regb:
                want64 = acc[:T, 0::2].double() * acc[:T, 1::2].double() * (inv * inv)[:, None]
                assert torch.equal(want.double(), want64), f"{what}: an expected value is not a {dtype} value"
            act = sent((tt_of(T) * 16 * I,), dtype, dev)
            o.lin.apply_ll(x[:T].to(dtype), fx=_fx(**kw), epi=2, out=act)
            same(act, fm_expected(want, tt_of(T)), what + " FM buffer")
            same(from_fm(act, T, I), want, what + " from_fm")


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,N,K,WK", EPI_CASES)
def test_ll_residual_epilogue_exact(dev, kind, N, K, WK, dtype):
    """epi 4: h (whole buffer), hw (whole FM buffer, arbitrary 16-bit norm_w), ssq_out group by group with sentinel columns behind
    the groups; norm_w = NULL leaves hw untouched; ssq_out = NULL is accepted"""
    awq = kind == "int4"
    R = _plan(N, K, awq)[0]
    groups = N // 16 // R
    g = torch.Generator().manual_seed(N + K)
    nw = (1 + 0.1 * torch.randn(N, generator=g)).to(dtype)
    h0a = (torch.randn(64, N, generator=g) * 8).to(dtype)                   # regime A: arbitrary 16-bit residual
    h0s = torch.randint(-3, 4, (64, N), generator=g).to(dtype)              # sums of squares: integer residual
    # regime A, dense: W in 0 .. 3 from K = 2048 on; below, W in 0 .. 15, so that the accumulators pass 2^11 in every plan
    oa = ll_lin(kind, N, K, dtype, dev, nonneg=not awq, wmax=WA if K >= 2048 else W_WIDE)
    os_ = ll_lin(kind, N, K, dtype, dev, s1=True) if awq else ll_lin(kind, N, K, dtype, dev)
    xa = xs_for(K, dev, nonneg=not awq)
    xs = xs_for(K, dev, nnz=NNZ_I4 if awq else SPARSE_NNZ)
    acc_a, acc_s = exact32(xa @ oa.Wd).cpu(), exact32(xs @ os_.Wd).cpu()
    differ = 0
    for T in T_EPI:
        what, TT = f"resid {kind} N={N} K={K} WK={WK} T={T}", tt_of(T)
        # regime A: two roundings on accumulators of many bits; no sums of squares asked for
        h, hw = h0a[:T].to(dev), sent((TT * 16 * N,), dtype, dev)
        oa.lin.apply_ll(xa[:T].to(dtype), fx=_fx(h=h, hw=hw, norm_w=nw.to(dev), ssq_out=None), epi=4)
        wh, whw = model_resid(acc_a[:T], h0a[:T], nw, dtype)
        differ += int((wh != model_resid(acc_a[:T], h0a[:T], nw, dtype, "one_rounding_in_the_residual_add")[0]).sum())
        same(h, wh, what + " A h")
        same(hw, fm_expected(whw, TT), what + " A hw")
        # integer h: sums of squares per row group, sentinel columns behind them
        h, hw = h0s[:T].to(dev), sent((TT * 16 * N,), dtype, dev)
        ssq = torch.full((T, groups + 3), -1.0, device=dev)
        os_.lin.apply_ll(xs[:T].to(dtype), fx=_fx(h=h, hw=hw, norm_w=nw.to(dev), ssq_out=ssq, ssq_out_stride=groups + 3), epi=4)
        wh, whw = model_resid(acc_s[:T], h0s[:T], nw, dtype)
        assert torch.equal(wh.double(), acc_s[:T].double() + h0s[:T].double()), what
        wssq = torch.full((T, groups + 3), -1.0)
        wssq[:, :groups] = group_ssq(wh, 16 * R)
        same(h, wh, what + " S h")
        same(hw, fm_expected(whw, TT), what + " S hw")
        same(ssq, wssq, what + " S ssq_out")
        # norm_w = NULL: hw untouched
        h, hw = h0s[:T].to(dev), sent((TT * 16 * N,), dtype, dev)
        os_.lin.apply_ll(xs[:T].to(dtype), fx=_fx(h=h, hw=hw, norm_w=None, ssq_out=None), epi=4)
        same(h, wh, what + " no norm_w h")
        same(hw, torch.full((TT * 16 * N,), SENT, dtype=dtype), what + " no norm_w hw")
    print(f"resid {kind} N={N} K={K} {dtype}: {differ} outputs tell two roundings from one, max acc {float(acc_a.max())}")
    assert differ > 0, "the regime A operands do not tell two roundings from one"


def qkv_operands(kind, Hq, Hkv, D, K, dtype, dev, regb):
    """(packed linear, x [64, K] float64, acc [64, N] fp32 on the CPU in HF feature order)"""
    N = (Hq + 2 * Hkv) * D
    awq = kind == "int4"
    key = ("lle-qkv", kind, N, K, D, dtype if kind == "dense" else None, regb)
    o = cached(key, lambda: pack(kind, *gen_w(kind, N, K, dev, 900 + N + K + regb, nonneg=not awq and not regb, s1=awq and regb),
                                 dtype, mode=(D, Hq + Hkv)))
    x = xs_for(K, dev, nnz=NNZ_QKV_B[kind], nonneg=False) if regb else xs_for(K, dev, nonneg=not awq)
    return o, x, cached(key + ("acc",), lambda: exact32(x @ o.Wd).cpu())


def qkv_tables(N, D, dtype, seed, P=96):
    g = torch.Generator().manual_seed(seed)
    cos, sin = torch.randn(P, D, generator=g).to(dtype), torch.randn(P, D, generator=g).to(dtype)     # arbitrary 16-bit tables
    return cos, sin, (torch.randn(N, generator=g) * 4).to(dtype), torch.randint(-3, 4, (N,), generator=g).to(dtype)


def check_qkv(run, acc, T, dtype, Hq, Hkv, D, Lmax, cos, sin, bias, regb, what, dev, rows=None):
    """one q/k/v launch against the model: q_out (whole buffer; `rows` > T: the rows behind T keep the sentinel) and the whole
    raw K / V^T storage, UMB_VT_PAD columns included"""
    pos, slot = pick_pos_slot(T, cos.shape[0], Lmax, T + D)
    kw, inv = {}, None
    if regb:
        ssq, _ = ssq_rows(T, 8, RMS_M_QKV)
        kw, inv = rms_kw(ssq.to(dev), 8), model_inv(ssq, 8)
        y = acc[:T].double() * inv[:, None] + (bias.double()[None] if bias is not None else 0.0)
        assert torch.equal(rnd(y.float(), dtype).double(), y), f"{what}: a pre-RoPE value is not a {dtype} value"
    q, k, v = model_qkv(acc[:T], dtype, pos, cos, sin, Hq, Hkv, D, inv=inv, bias=bias)
    wq = torch.full((rows or T, Hq, D), SENT, dtype=dtype)
    wq[:T] = q
    wk, wv = cache_expected(k, v, slot, Lmax)
    q_out, kc, vt = sent((rows or T, Hq, D), dtype, dev), sent((Hkv, Lmax, D), dtype, dev), sent((Hkv, D, Lmax + VT_PAD), dtype, dev)
    run(_fx(pos=pos.to(dev), slot=slot.to(dev), cosT=cos.to(dev), sinT=sin.to(dev), q_out=q_out, k_cache=kc, vt_cache=vt,
            Hq=Hq, Hkv=Hkv, D=D, Lmax=Lmax, bias=None if bias is None else bias.to(dev), **kw))
    same(q_out, wq, what + " q_out")
    same(kc, wk, what + " K storage")
    same(vt, wv, what + " V^T storage")
    return int((rope_single_rounded(acc[:T], dtype, pos, cos, sin, Hq, Hkv, D, bias) != torch.cat([q, k], 1)[..., :D // 2]).sum())


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,Hq,Hkv,D,K,WK", QKV_CASES)
def test_ll_qkv_epilogue_exact(dev, kind, Hq, Hkv, D, K, WK, dtype):
    """epi 3: (bias) + 1/rms + RoPE with arbitrary 16-bit tables + KV append, regimes A and B"""
    N, Lmax = (Hq + 2 * Hkv) * D, 128
    cos, sin, bias_a, bias_b = qkv_tables(N, D, dtype, N + K)
    differ = 0
    for regb in (False, True):
        o, x, acc = qkv_operands(kind, Hq, Hkv, D, K, dtype, dev, regb)
        for T in T_EPI:
            for bias in (None, bias_b if regb else bias_a):
                what = f"qkv {kind} ({Hq}, {Hkv}, {D}) K={K} WK={WK} T={T} regime {'B' if regb else 'A'} bias={bias is not None}"
                d = check_qkv(lambda fx: o.lin.apply_ll(x[:T].to(dtype), fx=fx, epi=3), acc, T, dtype, Hq, Hkv, D, Lmax, cos, sin,
                              bias, regb, what, dev)
                differ += 0 if regb else d
    assert differ > 0, "the regime A operands do not tell the two roundings of rotate-half from one"


# ------------------------------------------------------------------ 3. gv_kernel: every launch shape
def gv_rows(W16, mode=0, D=0, rope_heads=0):
    from umbrella_amd import _lib
    out = torch.empty_like(W16)
    _lib.call("umb_repack_rows", out, W16.contiguous(), W16.shape[0], W16.shape[1], mode, D, rope_heads)
    return out


def gemv(out, x16, rows, T, N, K, epi, fx):
    from umbrella_amd import _lib
    assert x16.shape == (T, K) and x16.is_contiguous()
    _lib.call("umb_gemv", out, x16, rows, T, N, K, epi, fx, _lib.dtype_code(x16.dtype))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K,passes", GV_RESID)
def test_gemv_residual_exact(dev, N, K, passes, dtype):
    """epi 4 at 1 .. 4 passes and both K: h and hw as whole 4-row buffers (rows >= T keep the sentinel), regime A with arbitrary h0
    and norm_w; integer h for the per-block sums of squares"""
    from umbrella_amd import _lib
    lib = _lib.load()
    assert gv_geometry(N, K, 4)[4] == passes
    g = torch.Generator().manual_seed(N + K)
    nw = (1 + 0.1 * torch.randn(N, generator=g)).to(dtype)
    h0a, h0s = (torch.randn(4, N, generator=g) * 8).to(dtype), torch.randint(-3, 4, (4, N), generator=g).to(dtype)
    Wa, Wda = gen_w("dense", N, K, dev, 1100 + N + K, nonneg=True)
    Ws, Wds = gen_w("dense", N, K, dev, 1200 + N + K)
    ra, rs = gv_rows(Wa.to(dtype)), gv_rows(Ws.to(dtype))
    xa, xs = xs_for(K, dev, nonneg=True)[:4], xs_for(K, dev, nnz=SPARSE_NNZ)[:4]
    acc_a, acc_s = exact32(xa @ Wda).cpu(), exact32(xs @ Wds).cpu()
    differ = 0
    for T in T_GV:
        what = f"gemv resid N={N} K={K} passes={passes} T={T}"
        groups = lib.umb_gemv_groups(T, N, K)
        assert groups == N // gv_geometry(N, K, 4)[3]
        # regime A
        h, hw = sent((4, N), dtype, dev), sent((4, N), dtype, dev)
        h[:T] = h0a[:T].to(dev)
        gemv(None, xa[:T].to(dtype).contiguous(), ra, T, N, K, 4, _fx(h=h, hw=hw, norm_w=nw.to(dev), ssq_out=None))
        wh, whw = model_resid(acc_a[:T], h0a[:T], nw, dtype)
        differ += int((wh != model_resid(acc_a[:T], h0a[:T], nw, dtype, "one_rounding_in_the_residual_add")[0]).sum())
        pad = torch.full((4 - T, N), SENT, dtype=dtype)
        same(h, torch.cat([wh, pad]), what + " A h")
        same(hw, torch.cat([whw, pad]), what + " A hw")
        # integer h, sums of squares per workgroup
        h, hw = sent((4, N), dtype, dev), sent((4, N), dtype, dev)
        h[:T] = h0s[:T].to(dev)
        ssq = torch.full((4, groups + 3), -1.0, device=dev)
        gemv(None, xs[:T].to(dtype).contiguous(), rs, T, N, K, 4,
             _fx(h=h, hw=hw, norm_w=nw.to(dev), ssq_out=ssq, ssq_out_stride=groups + 3))
        wh, whw = model_resid(acc_s[:T], h0s[:T], nw, dtype)
        assert torch.equal(wh.double(), acc_s[:T].double() + h0s[:T].double()), what
        wssq = torch.full((4, groups + 3), -1.0)
        wssq[:T, :groups] = group_ssq(wh, N // groups)
        same(h, torch.cat([wh, pad]), what + " S h")
        same(hw, torch.cat([whw, pad]), what + " S hw")
        same(ssq, wssq, what + " S ssq_out")
        # norm_w = NULL leaves hw untouched
        h, hw = sent((4, N), dtype, dev), sent((4, N), dtype, dev)
        h[:T] = h0s[:T].to(dev)
        gemv(None, xs[:T].to(dtype).contiguous(), rs, T, N, K, 4, _fx(h=h, hw=hw, norm_w=None, ssq_out=None))
        same(h, torch.cat([wh, pad]), what + " no norm_w h")
        same(hw, torch.full((4, N), SENT, dtype=dtype), what + " no norm_w hw")
    assert differ > 0, "the regime A operands do not tell two roundings from one"


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,K,passes", GV_SILU)
def test_gemv_silu_exact(dev, N, K, passes, dtype):
    """epi 2 at 1, 1, 2 and 4 passes: act as a whole 4-row buffer; regime A, and regime B for every group count of the
    four-values-per-lane read"""
    I = N // 2
    assert gv_geometry(N, K, 2)[4] == passes
    src, Wd = gen_silu_w("dense", I, K, dev, 1300 + N)
    rows = gv_rows(src.to(dtype), 1)
    il = torch.stack([torch.arange(I), I + torch.arange(I)], 1).reshape(-1).to(dev)
    for name, nnz, regb in silu_variants(dtype):
        x = xs_for(K, dev, nnz=nnz, nonneg=True)[:4]                          # K = 2048 >= every nnz
        acc = exact32(x @ Wd[:, il]).cpu()
        for T in T_GV:
            for G in (G_GV if regb else (0,)):
                what = f"gemv SiLU N={N} passes={passes} T={T} {name} G={G}"
                kw, inv = {}, None
                if regb:
                    ssq, _ = ssq_rows(T, G)
                    kw, inv = rms_kw(ssq.to(dev), G), model_inv(ssq, G)
                want = model_silu(acc[:T], dtype, inv=inv)
                silu_rounds(acc[:T], want, name)
                if regb:
                    want64 = acc[:T, 0::2].double() * acc[:T, 1::2].double() * (inv * inv)[:, None]
                    assert torch.equal(want.double(), want64), f"{what}: an expected value is not a {dtype} value"
                act = sent((4, I), dtype, dev)
                gemv(act, x[:T].to(dtype).contiguous(), rows, T, N, K, 2, _fx(**kw))
                same(act, torch.cat([want, torch.full((4 - T, I), SENT, dtype=dtype)]), what)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,Hq,Hkv,D,passes", GV_QKV)
def test_gemv_qkv_exact(dev, N, Hq, Hkv, D, passes, dtype):
    """epi 3: 6 of 8 slots (Llama-3.2-1B), two passes (D = 128: the second operand buffer), one pair per block; same buffers and
    conditions as the low-latency q/k/v test"""
    K, Lmax = 2048, 128
    assert gv_geometry(N, K, 3)[4] == passes
    cos, sin, bias_a, bias_b = qkv_tables(N, D, dtype, N + 1)
    differ = 0
    for regb in (False, True):
        W, Wd = gen_w("dense", N, K, dev, 1400 + N + regb, nonneg=not regb)
        rows = gv_rows(W.to(dtype), 2, D, Hq + Hkv)
        x = (xs_for(K, dev, nnz=NNZ_QKV_B["dense"]) if regb else xs_for(K, dev, nonneg=True))[:4]
        acc = exact32(x @ Wd).cpu()
        for T in T_GV:
            for bias in (None, bias_b if regb else bias_a):
                what = f"gemv qkv ({Hq}, {Hkv}, {D}) passes={passes} T={T} regime {'B' if regb else 'A'} bias={bias is not None}"
                d = check_qkv(lambda fx: gemv(None, x[:T].to(dtype).contiguous(), rows, T, N, K, 3, fx), acc, T, dtype, Hq, Hkv, D,
                              Lmax, cos, sin, bias, regb, what, dev, rows=4)
                differ += 0 if regb else d
    assert differ > 0, "the regime A operands do not tell the two roundings of rotate-half from one"


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi", [2, 3, 4])
def test_gemv_batch_invariance_every_epilogue(dev, epi, dtype):
    """a T-row launch is bitwise the 4-row launch's first T rows, on real-valued random operands"""
    from umbrella_amd import _lib
    g = _gen(dev, 1500 + epi)
    K, Hq, Hkv, D, Lmax = 2048, 32, 8, 64, 128
    N = {2: 4608, 3: (Hq + 2 * Hkv) * D, 4: 2304}[epi]
    rows = gv_rows((torch.randn(N, K, device=dev, generator=g) * 0.03).to(dtype), {2: 1, 3: 2, 4: 0}[epi], D, Hq + Hkv)
    x = torch.randn(4, K, device=dev, generator=g).to(dtype)
    ssq = torch.rand(4, 70, device=dev, generator=g) * 40 + 10
    h0 = torch.randn(4, N, device=dev, generator=g).to(dtype)
    nw = (1 + 0.1 * torch.randn(N, device=dev, generator=g)).to(dtype)
    bias = (torch.randn(N, device=dev, generator=g) * 0.1).to(dtype)
    ang = torch.rand(Lmax, D, device=dev, generator=g) * 6.28
    cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
    pos = torch.tensor([5, 0, 127, 64], dtype=torch.int32, device=dev)
    slot = torch.tensor([33, 0, 127, 31], dtype=torch.int32, device=dev)
    rkw = dict(ssq_in=ssq, ssq_groups=65, ssq_in_stride=70, ssq_dim=float(K), eps=1e-5)
    groups = _lib.load().umb_gemv_groups(4, N, K)

    def run(T):
        xt = x[:T].contiguous()
        if epi == 2:
            act = sent((4, N // 2), dtype, dev)
            gemv(act, xt, rows, T, N, K, 2, _fx(**rkw))
            return [act[:T]]
        if epi == 4:
            h, hw, so = h0.clone(), sent((4, N), dtype, dev), torch.zeros(4, groups, device=dev)
            gemv(None, xt, rows, T, N, K, 4, _fx(h=h, hw=hw, norm_w=nw, ssq_out=so, ssq_out_stride=groups))
            return [h[:T], hw[:T], so[:T]]
        q, kc, vt = sent((4, Hq, D), dtype, dev), sent((Hkv, Lmax, D), dtype, dev), sent((Hkv, D, Lmax + VT_PAD), dtype, dev)
        gemv(None, xt, rows, T, N, K, 3, _fx(pos=pos[:T].contiguous(), slot=slot[:T].contiguous(), cosT=cos, sinT=sin, q_out=q,
                                            k_cache=kc, vt_cache=vt, Hq=Hq, Hkv=Hkv, D=D, Lmax=Lmax, bias=bias, **rkw))
        sl = slot[:T].long()
        return [q[:T], kc.view(Hkv, -1)[:, k_offsets(sl, D)], vt.view(Hkv, -1)[:, vt_offsets(sl, D)]]
    full = run(4)
    for T in (1, 2, 3):
        part = run(T)
        for i, (a, b) in enumerate(zip(part, full)):
            if epi == 3 and i > 0:
                b = b[:, :T] if i == 1 else b[:, :, :T]
            else:
                b = b[:T]
            assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
                                                      b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32)), (epi, T, i)
        assert float(part[0].float().abs().max()) > 0


# ------------------------------------------------------------------ 4. contracts
@gpu
def test_contract_refusals(dev):
    """every refused launch returns UMB_EINVAL and leaves its sentinel-filled buffers untouched"""
    from umbrella_amd import _lib
    lib = _lib.load()
    st = _lib.stream_ptr()
    # valid operands of generous size: a refusal that regressed would run in bounds (pos and slot are zeros) and show up as a
    # modified sentinel, not as a fault
    w = torch.zeros(64 << 20, dtype=torch.uint8, device=dev)                    # weights and metadata
    x = torch.zeros(1 << 20, dtype=F16, device=dev)
    idx = torch.zeros(128, dtype=torch.int32, device=dev)                       # pos, slot
    tab = torch.ones(1 << 16, dtype=F16, device=dev)                            # cos, sin, norm_w
    ssq_in = torch.ones(1 << 16, dtype=torch.float32, device=dev)
    outs = {"out": torch.full((1 << 20,), NAN, dtype=torch.float32, device=dev), "ssq_out": torch.full((1 << 16,), -1.0, device=dev)}
    outs.update({k: sent((1 << 20,), F16, dev) for k in ("h", "hw", "q_out", "k_cache", "vt_cache")})
    keep = {k: v.clone() for k, v in outs.items()}
    P = _lib.ptr
    dt = _lib.dtype_code(F16)
    ptrs = dict(h=outs["h"], hw=outs["hw"], norm_w=tab, ssq_out=outs["ssq_out"], pos=idx, slot=idx, cosT=tab, sinT=tab,
                q_out=outs["q_out"], k_cache=outs["k_cache"], vt_cache=outs["vt_cache"])

    def ll(T=4, N=64, K=128, awq=0, epi=0, meta=True, **kw):
        fx = _fx(**kw)
        return lib.umb_gemm_ll(P(outs["out"]), P(x), P(w), P(w) if meta else None, T, N, K, awq, epi, C.byref(fx), dt, st)
    qkv = dict(Hq=2, Hkv=1, D=32, Lmax=64, **ptrs)                              # N = 128
    bad_ll = {
        "row_from < 0": ll(row_from=-1), "row_from >= T": ll(row_from=4),
        "ssq_in_stride < ssq_groups": ll(ssq_in=ssq_in, ssq_groups=8, ssq_in_stride=4, ssq_dim=128.0),
        "ssq_dim <= 0": ll(ssq_in=ssq_in, ssq_groups=8, ssq_in_stride=8, ssq_dim=0.0),
        "awq = 2": ll(awq=2), "int4 N % 64": ll(N=80, awq=1), "int4 without meta": ll(awq=1, meta=False),
        "resid ssq_out_stride below the groups": ll(epi=4, ssq_out_stride=3, **ptrs),
        "qkv D % 32": ll(N=64, epi=3, **dict(qkv, D=16)), "qkv Lmax % 32": ll(N=128, epi=3, **dict(qkv, Lmax=48)),
        "qkv Lmax < 32": ll(N=128, epi=3, **dict(qkv, Lmax=0)), "qkv N != (Hq + 2 Hkv) D": ll(N=160, epi=3, **qkv),
        "silu N % 32": ll(N=48, epi=2), "T = 0": ll(T=0), "T = 65": ll(T=65),
    }

    def gv(T=2, N=2048, K=2048, epi=4, **kw):
        fx = _fx(**dict(ptrs, **kw))
        return lib.umb_gemv(P(outs["out"]), P(x), P(w), T, N, K, epi, C.byref(fx), dt, st)
    bad_gv = {
        "T = 5": gv(T=5, ssq_out_stride=256), "K = 4096": gv(K=4096, ssq_out_stride=256),
        "K = 8192 epi 2": gv(K=8192, epi=2), "K = 8192 epi 3": gv(K=8192, epi=3, Hq=24, Hkv=4, D=64, Lmax=64),
        "ssq_groups = 0": gv(epi=2, ssq_in=ssq_in, ssq_groups=0, ssq_dim=2048.0),
        "ssq_groups = 257": gv(epi=2, ssq_in=ssq_in, ssq_groups=257, ssq_dim=2048.0),
        "resid ssq_out_stride below the blocks": gv(ssq_out_stride=255),
        "qkv D % 32": gv(epi=3, Hq=96, Hkv=16, D=16, Lmax=64), "qkv Lmax % 32": gv(epi=3, Hq=24, Hkv=4, D=64, Lmax=48),
    }
    torch.cuda.synchronize()
    wrong = {k: v for k, v in {**bad_ll, **{"gemv " + k: v for k, v in bad_gv.items()}}.items() if v != EINVAL}
    assert not wrong, wrong
    for k, v in outs.items():
        same(v, keep[k], f"a refused launch wrote to {k}")


# ------------------------------------------------------------------ 5. CPU: the reference as a model, one seeded defect per run
DEFECTS = ["wk_sibling_partial_dropped", "ssq_groups_beyond_64_ignored", "inv_from_token_t_plus_1", "gate_and_up_swapped_in_a_pair",
           "sign_of_sin_on_the_low_half", "slot_of_the_neighbouring_token", "row_from_off_by_one", "hw_from_h_before_the_add",
           "one_rounding_in_the_residual_add"]


def run_model(defect, dtype=F16, T=17):
    """the epilogue path the defect lives in, on this module's operand generators (CPU): a list of output buffers"""
    cpu = torch.device("cpu")
    N, K, WK = 64, 512, 4
    if defect in (None, "wk_sibling_partial_dropped", "inv_from_token_t_plus_1", "row_from_off_by_one"):
        _, Wd = gen_w("dense", N, K, cpu, 1)
        acc = model_acc(int_x(T, K, cpu, 2, nnz=SPARSE_NNZ), Wd, WK, defect)
        ssq, _ = ssq_rows(T, 33)
        yield model_logits(acc, T, dtype, inv=model_inv(ssq, 33, defect), round_out=True, row_from=1, defect=defect)
    if defect in (None, "ssq_groups_beyond_64_ignored", "gate_and_up_swapped_in_a_pair"):
        I = 32
        _, Wd = gen_silu_w("dense", I, K, cpu, 3)
        il = torch.stack([torch.arange(I), I + torch.arange(I)], 1).reshape(-1)
        acc = model_acc(int_x(4, K, cpu, 4, nnz=NNZ_SILU_B).abs(), Wd[:, il])
        ssq, _ = ssq_rows(4, 65)
        yield fm_expected(model_silu(acc, dtype, inv=model_inv(ssq, 65, defect), defect=defect), 1)
    if defect in (None, "sign_of_sin_on_the_low_half", "slot_of_the_neighbouring_token"):
        Hq, Hkv, D, Lmax = 2, 1, 32, 64
        _, Wd = gen_w("dense", (Hq + 2 * Hkv) * D, K, cpu, 5, nonneg=True)
        acc = model_acc(int_x(T, K, cpu, 6).abs(), Wd)
        cos, sin, bias, _ = qkv_tables((Hq + 2 * Hkv) * D, D, dtype, 7)
        pos, slot = pick_pos_slot(T, cos.shape[0], Lmax, 8)
        q, k, v = model_qkv(acc, dtype, pos, cos, sin, Hq, Hkv, D, bias=bias, defect=defect)
        yield q
        yield from cache_expected(k, v, slot, Lmax, defect)
    if defect in (None, "hw_from_h_before_the_add", "one_rounding_in_the_residual_add"):
        _, Wd = gen_w("dense", N, 2048, cpu, 9, nonneg=True)
        acc = model_acc(int_x(T, 2048, cpu, 10).abs(), Wd)
        g = torch.Generator().manual_seed(11)
        h0, nw = (torch.randn(T, N, generator=g) * 8).to(dtype), (1 + 0.1 * torch.randn(N, generator=g)).to(dtype)
        h, hw = model_resid(acc, h0, nw, dtype, defect)
        yield h
        yield fm_expected(hw, tt_of(T))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", DEFECTS)
def test_every_seeded_defect_fails_the_exact_comparison(defect, dtype):
    want = {id_: b for id_, b in enumerate(run_model(None, dtype))}
    again = list(run_model(None, dtype))
    for i, b in want.items():
        same(again[i], b, "the model against itself")
    # the buffers of the defect's own path, in the order run_model(None) yields them
    first = {"wk_sibling_partial_dropped": 0, "inv_from_token_t_plus_1": 0, "row_from_off_by_one": 0, "ssq_groups_beyond_64_ignored": 1,
             "gate_and_up_swapped_in_a_pair": 1, "sign_of_sin_on_the_low_half": 2, "slot_of_the_neighbouring_token": 2,
             "hw_from_h_before_the_add": 5, "one_rounding_in_the_residual_add": 5}[defect]
    got = list(run_model(defect, dtype))
    caught = 0
    for i, b in enumerate(got):
        try:
            same(b, want[first + i], defect)
        except AssertionError as e:
            assert "values differ" in str(e)
            caught += 1
    assert caught >= 1, f"{defect} passes the exact comparison"


def test_which_defects_the_relative_metric_lets_through():
    """the record of what this module adds: `max|a - b| / max|b| < 2e-2` (the widest bound of tests/test_lowlat.py and
    tests/test_gemv.py) on the same buffers.  Printed and reported, not asserted."""
    first = {"wk_sibling_partial_dropped": 0, "inv_from_token_t_plus_1": 0, "row_from_off_by_one": 0, "ssq_groups_beyond_64_ignored": 1,
             "gate_and_up_swapped_in_a_pair": 1, "sign_of_sin_on_the_low_half": 2, "slot_of_the_neighbouring_token": 2,
             "hw_from_h_before_the_add": 5, "one_rounding_in_the_residual_add": 5}
    want = list(run_model(None, BF16))
    passed = []
    for d in DEFECTS:
        worst = 0.0
        for i, b in enumerate(run_model(d, BF16)):
            w = torch.nan_to_num(want[first[d] + i].float(), nan=0.0)
            worst = max(worst, float((torch.nan_to_num(b.float(), nan=0.0) - w).abs().max() / w.abs().max().clamp_min(1e-6)))
        print(f"defect {d}: rel {worst:.3e} -> {'PASSES' if worst < 2e-2 else 'fails'} the 2e-2 metric")
        if worst < 2e-2:
            passed.append(d)
    print("defects the relative metric lets through:", passed)
    try:
        from conftest import report_fact
        report_fact("lowlat_exact.defects_the_relative_metric_passes", passed)
    except ImportError:
        pass


def test_rounding_discrimination_counts():
    """T = 16, N = 512, K = 2048, x and W uniform in 0 .. 3: how many outputs tell rnd(rnd(acc) + h) from rnd(acc + h), and
    rnd(rnd(a c) + rnd(-b s)) from the single-rounded sum (a, b integers in +-144, random cos / sin).  Non-zero per dtype."""
    cpu = torch.device("cpu")
    _, Wd = gen_w("dense", 512, 2048, cpu, 21, nonneg=True)
    acc = exact32(int_x(16, 2048, cpu, 22).abs() @ Wd)
    g = torch.Generator().manual_seed(23)
    facts = {}
    for dtype, name in ((F16, "f16"), (BF16, "bf16")):
        h0 = (torch.randn(16, 512, generator=g) * 8).to(dtype)
        two = model_resid(acc, h0, None, dtype)[0]
        one = model_resid(acc, h0, None, dtype, "one_rounding_in_the_residual_add")[0]
        facts[f"residual_{name}"] = int((two != one).sum())
        a = torch.randint(-144, 145, (16, 512), generator=g).float()                        # (Hq, Hkv, D) = (4, 2, 64)
        cos, sin = torch.randn(96, 64, generator=g).to(dtype), torch.randn(96, 64, generator=g).to(dtype)
        pos = torch.randint(0, 96, (16,), generator=g, dtype=torch.int32)
        q, k, _ = model_qkv(a, dtype, pos, cos, sin, 4, 2, 64)
        single = rope_single_rounded(a, dtype, pos, cos, sin, 4, 2, 64)
        facts[f"rope_{name}"] = int((single != torch.cat([q, k], 1)[..., :32]).sum())
    print("rounding discrimination:", facts)
    assert all(v > 0 for v in facts.values()), facts
    try:
        from conftest import report_fact
        for k, v in facts.items():
            report_fact("lowlat_exact.two_roundings_differ_from_one." + k, v)
    except ImportError:
        pass
