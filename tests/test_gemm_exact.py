"""Exact GEMM tests: every split slab of every kernel family, bit for bit against a float64 matmul.

Operands are chosen so that fp32 accumulation is exact IN ANY ORDER; the kernels (csrc/gemm.hip, vgemm.hip, lowlat.hip,
gemv.hip, the streamed head of chain.hip) then have no freedom left, and each partial slab out[s] must equal the sum
over exactly its own k range [s * per, min(KB, (s + 1) * per)) * 128, per = ceil(KB / S) -- an EMPTY range is a slab of
zeros (include/umbrella_hip.h: umb_gemm).

Why the sums are exact (every bound below is evaluated by test_exactness_bounds for each (K, range) the module uses):

  dense      x, W integers with |x| <= XA = 3, |W| <= WA = 3 (exact in fp16 and bf16).  Every product is an integer,
             every partial sum of any subset of the K terms is an integer of magnitude <= K * XA * WA < 2^24.
  int4       q, z arbitrary codes in 0 .. 15, scales s = 2^e with e from SCALE_EXPS per (group, column), so
             (q - z) * s is exact in fp16 and the exact-dequant form (gemm.hip AWQ == 2, vgemm.hip) and the folded
             form s * (sum q x - z sum x) (gemm.hip AWQ == 1, lowlat.hip) give the same number.
             Inside one 128-k group the folded kernels run the MFMA on OFFSET codes C + q and cancel C afterwards:
               gemm.hip stage_compute: C = 64 (fp16, 0x5400 | nibble << 4) or 128 (bf16, 0x4300 | nibble); the chain
                 starts from -C * sum x and adds 128 terms (C + q) x: any partial sum is an integer of magnitude
                 <= 128 * C * XA + 128 * (C + 15) * XA;
               lowlat.hip compute: C = 1024 and 64 (fp16), 128 (bf16); sum (C + q) x and -sum C x are separate chains
                 of <= 128 * (1024 + 15) * XA each, added afterwards;
             both far below 2^24 for XA = 3.  Then t = sum q x - z sum x is an integer, |t| <= 128 * 15 * XA, and
             acc += s * t: every partial sum over groups is a multiple of 2^min(SCALE_EXPS) of magnitude
             <= K * 15 * XA * 2^max(SCALE_EXPS), i.e. < 2^24 units as long as K * 15 * XA * 2^(max - min) < 2^24.
  16-bit out where a kernel ROUNDS its result to the model dtype (epi 1, the GEMV residual epilogue, the streamed head) the
             activations are sparse (SPARSE_NNZ non-zeros per row), so |out| <= SPARSE_NNZ * XA * WA < 256: an integer
             that bf16 (8 significant bits) and fp16 hold exactly.

  1/rms     the per-token factor rsqrt(sum ssq / dim + eps) of the fused RMSNorm consumers (epi 1, 2) is made a power of two:
             sums of squares K * 4^m / 8 in 8 groups, dim = K, eps = 0 give 2^-m with m in RMS_M.  acc * 2^-m keeps acc's
             significand, and |acc| <= SPARSE_NNZ * XA * max(WA, 15) on sparse rows (int4 at scale 1.0), so every expected
             output is a 16-bit value (test_token_rms_bounds).

One-hot rows (x[t] = e_k) read the repacked weights back with no summation at all, so they may use REAL fp16 scales and pin
the two dequant contracts: exact form out = fp32(fp16((q - z) * s)); folded form out = fp32(s) * fp32(q - z) (a 15-bit
product, exact in fp32; the chain -C + (C + q) = q and t = q - z are exact).  SiLU(gate) * up (epi 2) on one-hot rows:
gates are 0 or GATE_ON = 32, for which g / (1 + exp(-g)) IS g in fp32 (test_silu_is_the_identity_on_the_gate_set), ups are
integers |u| <= 3, so the activation is exactly gate * up.

CPU part (no gpu mark): the bounds, the packing helper, the SiLU identity and a numpy model of a tiled split-K int4 GEMM with
one seeded defect each -- every defect must fail this module's assertion helper; which of them the older
`max|a - b| / max|b| < 2e-3` metric lets through is printed (run with -s), not asserted.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

XA, WA = 3, 3                        # |x|, |dense W| (integers)
SCALE_EXPS = (-6, -5, -4, -3)        # int4 scales 2^e
SPARSE_NNZ = 16                      # non-zeros per row where the output is rounded to 16 bits
GATE_ON = 32.0                       # the non-zero gate value of the SiLU probes
RMS_M = (-1, 0, 1)                   # per-token exponents m of the sums of squares: 1/rms = 2^-m = 2, 1, 0.5
RMS_G, RMS_STRIDE = 8, 12            # valid groups per ssq row, row stride (the columns behind the groups are never read)
T_RMS = (129, 193, 257)              # one wide chunk + a skinny tail; a tail above 64 (all wide); the 144-token items
T_SKINNY = (1, 15, 16, 17, 31, 32, 33, 48, 63, 64)
T_WIDE = (65, 128, 129, 192, 193, 256, 257, 300, 385)
S_SKINNY = (1, 3, 5, 6, 7, 16)       # KB = 16: whole, ragged (6 6 4), empty trailing (4 x 4 + 0), 3 3 3 3 3 1, empty + 1-block, 1-block
K_SMALL = 2048
# every (K, form) the GPU tests below use: test_exactness_bounds evaluates the docstring's bounds for each
USED_SHAPES = [(384, "int4"), (512, "dense"), (512, "int4"), (2048, "dense"), (2048, "int4"), (4096, "dense"), (4096, "int4"),
               (8192, "int4")]
# magic offsets C of the folded kernels (read from Stage / stage_compute in gemm.hip and compute() in lowlat.hip)
OFFSETS = {"gemm.hip fp16": (64,), "gemm.hip bf16": (128,), "lowlat.hip fp16": (1024, 64), "lowlat.hip bf16": (128,)}


# ------------------------------------------------------------------ bounds (CPU)
def chain_bound(C, xa=XA):
    """largest magnitude any partial sum of one 128-k group's offset-code chain can reach (start value -C sum x included)"""
    return 128 * C * xa + 128 * (C + 15) * xa


def acc_units(K, form, xa=XA, wa=WA):
    """largest magnitude of any partial sum of the K terms, in units of the smallest representable step"""
    if form == "dense":
        return K * xa * wa
    return K * 15 * xa * 2 ** (max(SCALE_EXPS) - min(SCALE_EXPS))


@pytest.mark.parametrize("K,form", USED_SHAPES)
def test_exactness_bounds(K, form):
    assert acc_units(K, form) < 2 ** 24, (K, form, acc_units(K, form))
    if form == "int4":
        for name, cs in OFFSETS.items():
            for C in cs:
                assert chain_bound(C) < 2 ** 24, (name, C)
        assert 128 * 15 * XA < 2 ** 24
        # (q - z) * s in fp16: 4 significant bits, normal range
        assert 15 * 2.0 ** max(SCALE_EXPS) < 65504 and 2.0 ** min(SCALE_EXPS) >= 2.0 ** -14
    # operands are exact in both 16-bit formats (bf16: 8 significant bits), and so is every rounded output
    for dt in (torch.float16, torch.bfloat16):
        v = torch.arange(-256, 257, dtype=torch.float32)
        assert torch.equal(v.to(dt).float(), v)
    assert SPARSE_NNZ * XA * WA <= 256 and GATE_ON * 3 <= 256


def test_token_rms_bounds():
    """test_wide_epilogues_apply_token_rms_exactly: acc * 2^-m has acc's significand, so it is a 16-bit value as soon as
    |acc| < 2^(significant bits) and the scaled value stays in the normal range."""
    assert SPARSE_NNZ * XA * WA < 2 ** 8                          # dense: bf16 holds 8 significant bits, fp16 11
    assert SPARSE_NNZ * XA * 15 < 2 ** 11                         # int4 at scale 1.0, |q - z| <= 15: fp16 only
    for m in RMS_M:
        assert SPARSE_NNZ * XA * 15 * 2.0 ** -m < 65504 and 2.0 ** -m >= 2.0 ** -14      # largest / smallest non-zero |acc * inv|
        for K in (512, K_SMALL):                                  # the groups and their sum are powers of two: exact in fp32
            v = np.float32(K * 4.0 ** m / RMS_G)
            assert float(v) * RMS_G == K * 4.0 ** m and float(np.float32(float(v) * RMS_G) / np.float32(K)) == 4.0 ** m
    # SiLU: gates 32 * {1, 2} stay >= 32 (the identity), gate * up * inv^2 <= 32 * 3 * 4 = 3 * 2^7: two significant bits
    for f in (1.0, 2.0):
        assert GATE_ON * f >= 32.0
        for u in range(-3, 4):
            for dt in (torch.float16, torch.bfloat16):
                assert float(torch.tensor(GATE_ON * u * f * f).to(dt)) == GATE_ON * u * f * f
    # a last-bit error of the hardware rsqrt / divide (2^-23 relative) against half an ulp of the 16-bit formats
    assert 4 * 2.0 ** -23 < 2.0 ** -12


def test_silu_is_the_identity_on_the_gate_set():
    """the kernels' formula g / (1 + __expf(-g)) in fp32: 1 + e == 1 for every e <= 2^-25, and exp(-32) is eleven orders
    below that, whatever the last bits of the fast exponential; g = 0 gives 0 / 2 = 0."""
    one = np.float32(1.0)
    for e in (np.float32(2.0 ** -25), np.float32(np.exp(np.float32(-GATE_ON))), np.float32(np.exp(np.float32(-GATE_ON)) * 1.01)):
        assert one + e == one
    assert float(np.exp(-GATE_ON)) * 1e6 < 2.0 ** -25
    g = np.float32(GATE_ON)
    assert g / (one + np.float32(np.exp(-g))) == g
    assert np.float32(0.0) / (one + np.float32(np.exp(np.float32(-0.0)))) == 0.0
    for u in range(-3, 4):           # gate * up is exact in 16 bits
        for dt in (torch.float16, torch.bfloat16):
            assert float(torch.tensor(GATE_ON * u).to(dt)) == GATE_ON * u


# ------------------------------------------------------------------ the assertion helper
def slab_range(KB, S, s):
    per = (KB + S - 1) // S
    return min(KB, s * per), min(KB, (s + 1) * per)


def assert_same_bits(got, want, what=""):
    """whole buffers, bit for bit; on failure the first differences as (split, row, column, got, want) and the 16 x 16 tiles
    that hold any"""
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    it = {4: torch.int32, 2: torch.int16, 8: torch.int64}[got.element_size()]
    g, w = got.contiguous().view(it), want.contiguous().view(it)
    if torch.equal(g, w):
        return
    bad = (g != w).nonzero()
    n = int(bad.shape[0])
    b3 = bad if bad.shape[1] == 3 else torch.cat([torch.zeros(n, 3 - bad.shape[1], dtype=bad.dtype, device=bad.device), bad], 1)
    first = [(*[int(v) for v in b3[i]], float(got[tuple(bad[i])]), float(want[tuple(bad[i])])) for i in range(min(n, 6))]
    tiles = torch.unique(torch.stack([b3[:, 0], b3[:, 1] // 16, b3[:, 2] // 16], 1), dim=0)
    raise AssertionError(f"{what}: {n} of {g.numel()} values differ; first (split, row, col, got, want): {first}; "
                         f"{int(tiles.shape[0])} wrong (split, token tile, n tile): {tiles[:12].tolist()}")


# ------------------------------------------------------------------ operands
ORDER = (0, 2, 4, 6, 1, 3, 5, 7)


def pack_rows_t(v):
    """awq_format.pack_rows on a torch tensor (any device): uint8 [R, N] -> int32 [R, N / 8]"""
    R, N = v.shape
    v = v.view(R, N // 8, 8).to(torch.int64)
    out = torch.zeros(R, N // 8, dtype=torch.int64, device=v.device)
    for i, col in enumerate(ORDER):
        out |= (v[:, :, col] & 0xF) << (4 * i)
    return ((out + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)


def test_pack_rows_t_equals_the_numpy_packer():
    from umbrella_amd.models.awq_format import pack_rows
    v = np.random.RandomState(0).randint(0, 16, size=(5, 64)).astype(np.uint8)
    assert np.array_equal(pack_rows_t(torch.from_numpy(v)).numpy(), pack_rows(v))


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def int_x(T, K, dev, seed, ld=None, nnz=None):
    """integer activations in [-XA, XA] as float64 [T, K] (nnz: that many non-zeros per row, at row-dependent places)"""
    g = _gen(dev, seed)
    x = torch.randint(-XA, XA + 1, (T, K), device=dev, generator=g).double()
    if nnz:
        keep = torch.zeros(T, K, dtype=torch.bool, device=dev)
        idx = torch.rand(T, K, device=dev, generator=g).argsort(1)[:, :nnz]
        keep.scatter_(1, idx, True)
        x = x * keep
    return x


def strided(x, dtype, pad=64):
    """[T, K] values as a view with row stride K + pad inside a buffer of sentinel values"""
    T, K = x.shape
    buf = torch.full((T + 3, K + pad), 7.0, dtype=dtype, device=x.device)
    buf[:T, :K] = x.to(dtype)
    return buf[:T, :K]


class Lin:
    """packed weights + their exact float64 values Wd [K, N] in OUTPUT column order"""
    pass


def perm_il(N, dev):
    n = torch.arange(N, device=dev)
    return torch.where(n % 2 == 1, N // 2 + n // 2, n // 2)             # packed row n <- source row (gemm.hip rowmap, mode 1)


def mk_dense(N, K, dtype, dev, seed, il=False, W=None):
    from umbrella_amd.models.llama import PackedLinear
    if W is None:
        W = torch.randint(-WA, WA + 1, (N, K), device=dev, generator=_gen(dev, seed)).double()
    o = Lin()
    o.lin = PackedLinear.from_dense(W.to(dtype), interleave=il)
    o.rows = W.to(dtype)
    o.Wd = (W[perm_il(N, dev)] if il else W).t().contiguous()
    o.N, o.K, o.awq = N, K, 0
    return o


def mk_int4(N, K, dev, seed, il=False, real_scales=False, q=None, z=None, s=None):
    from umbrella_amd.models.llama import PackedLinear
    g = _gen(dev, seed)
    if q is None:
        q = torch.randint(0, 16, (K, N), device=dev, generator=g, dtype=torch.uint8)
        z = torch.randint(0, 16, (K // 128, N), device=dev, generator=g, dtype=torch.uint8)
        if s is not None:
            pass                                                            # generated codes under the caller's scales
        elif real_scales:
            s = (torch.rand(K // 128, N, device=dev, generator=g) * 0.02 + 0.002).half()
        else:
            e = torch.randint(0, len(SCALE_EXPS), (K // 128, N), device=dev, generator=g)
            s = torch.tensor([2.0 ** v for v in SCALE_EXPS], device=dev)[e].half()
    o = Lin()
    o.lin = PackedLinear.from_awq(pack_rows_t(q), pack_rows_t(z), s, interleave=il)
    d = q.double() - z.double().repeat_interleave(128, 0)               # q - z, [K, N]
    sr = s.double().repeat_interleave(128, 0)
    o.d, o.s = d, sr
    o.Wd = d * sr
    if il:
        p = perm_il(N, dev)
        o.Wd, o.d, o.s = o.Wd[:, p], d[:, p], sr[:, p]
    o.N, o.K, o.awq = N, K, 1
    return o


def slab_refs(x64, Wd, S):
    """fp32 [S, T, N]: slab s = x[:, k0:k1] . W[k0:k1] in float64 (exact), which fp32 holds exactly by the bounds"""
    T, K = x64.shape
    KB = K // 128
    out = torch.zeros(S, T, Wd.shape[1], dtype=torch.float64, device=x64.device)
    for s in range(S):
        k0, k1 = slab_range(KB, S, s)
        if k1 > k0:
            out[s] = x64[:, k0 * 128:k1 * 128] @ Wd[k0 * 128:k1 * 128]
    f = out.float()
    assert torch.equal(f.double(), out)
    return f


def run_gemm(o, x, T, S, Rtb, epi=0, fx=None, out=None):
    from umbrella_amd import _lib
    if out is None:
        out = torch.full((S, T, o.N), float("nan"), dtype=torch.float32, device=x.device)
    args = (out, x, x.stride(0) if x.dim() == 2 else o.K, o.lin.w, o.lin.meta, T, o.N, o.K, o.awq, S, Rtb, epi)
    if fx is None:
        _lib.call("umb_gemm", *args, _lib.dtype_code(x.dtype))
    else:
        _lib.call("umb_gemm_fused", *args, fx, _lib.dtype_code(x.dtype))
    return out


class env:
    """environment variables the library reads per call, restored on exit"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from umbrella_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


FORMS = {"dense-f16": ("dense", torch.float16, None), "dense-bf16": ("dense", torch.bfloat16, None),
         "folded-f16": ("int4", torch.float16, None), "folded-bf16": ("int4", torch.bfloat16, None),
         "exact-f16": ("int4", torch.float16, "exact")}


def small_lin(form, dev):
    kind, dtype, _ = FORMS[form]
    # N: 62 n-tiles dense / 60 int4 (int4 rows come in groups of 64): the last block is ragged for every tb below except
    # R = 1 at 4 / 5 / 6 tiles of the int4 matrix, and with tb = 7 every second block starts on an odd tile
    if kind == "dense":
        return cached(("dense", dtype), lambda: mk_dense(992, K_SMALL, dtype, dev, 11))
    return cached(("int4",), lambda: mk_int4(960, K_SMALL, dev, 12))


def small_x(dev):
    return cached(("x64",), lambda: int_x(64, K_SMALL, dev, 5))


# R | tb << 8 words: default, R = 2, tb = 7 with R = 2, 8 waves x 2 tiles (folded int4 at <= 16 rows; every other launch runs
# the same balance as 4-wave blocks of 7), 8 waves x 1 tile at 5 .. 8 tiles per block.  At these sizes the launcher takes the word as
# given: the plan's own condition for the 8-wave forms, (NT / t) * S == 256, is met only at full size (test_full_size_*).
VARIANTS = {"r1": 1, "r2": 2, "r2tb7": 2 | 7 << 8, "r2tb14w8": 2 | (14 | 0x80) << 8, "r1tb5w8": 1 | (5 | 0x80) << 8,
            "r1tb6w8": 1 | (6 | 0x80) << 8, "r1tb7w8": 1 | (7 | 0x80) << 8, "r1tb8w8": 1 | (8 | 0x80) << 8}


# ------------------------------------------------------------------ 1. skinny kernel, T <= 64
@gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("form", list(FORMS))
def test_skinny_every_slab_bit_for_bit(dev, form, variant):
    kind, dtype, dq = FORMS[form]
    o, x64 = small_lin(form, dev), small_x(dev)
    refs = {S: cached((form[:5] == "dense", "ref", S), lambda: slab_refs(x64, o.Wd, S)) for S in S_SKINNY}
    n = 0
    with env(UMB_DEQUANT=dq):
        for T in T_SKINNY:
            x = strided(x64[:T], dtype) if T % 3 else x64[:T].to(dtype).contiguous()      # ldx > K and ldx == K in every tile class
            for S in S_SKINNY:
                got = run_gemm(o, x, T, S, VARIANTS[variant])
                assert_same_bits(got, refs[S][:, :T].contiguous(), f"{form} {variant} T={T} S={S} ldx={x.stride(0)}")
                n += 1
    assert n == len(T_SKINNY) * len(S_SKINNY)


@gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_skinny_fm_activations_equal_row_major(dev, form):
    """x in FM (MFMA B-fragment) order in, row-major partials out: the same bits as the row-major launch and the reference"""
    from umbrella_amd import _lib
    from umbrella_amd.models.llama import to_fm
    kind, dtype, dq = FORMS[form]
    o, x64 = small_lin(form, dev), small_x(dev)
    fx = _lib.UmbGemmFused()
    fx.pad1 = 1
    with env(UMB_DEQUANT=dq):
        for T in T_SKINNY:
            for S, Rtb in ((1, 1), (5, 1), (3, 2), (16, VARIANTS["r1tb7w8"])):
                want = slab_refs(x64[:T], o.Wd, S)
                got = run_gemm(o, to_fm(x64[:T].to(dtype)), T, S, Rtb, fx=fx)
                assert_same_bits(got, want, f"{form} FM T={T} S={S} Rtb={Rtb:#x}")


@gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_skinny_two_blocks_per_cu_launch(dev, dtype):
    """nblk * S == 512 four-wave blocks: the launch that asks for 56 KiB of LDS so that no CU admits a third block"""
    o = cached(("dense2048", dtype), lambda: mk_dense(2048, K_SMALL, dtype, dev, 13))
    x64 = small_x(dev)
    for T in (13, 40):
        assert_same_bits(run_gemm(o, strided(x64[:T], dtype), T, 16, 1), slab_refs(x64[:T], o.Wd, 16), f"{dtype} T={T}")


# ------------------------------------------------------------------ 2. T > 64
def wide_x(dev, K):
    return cached(("xw", K), lambda: int_x(512, K, dev, 6 + K))


def wide_case(dev, name):
    """(weights, [(S, environment)]) of one wide configuration; see WIDE for which kernel each one reaches"""
    f16, bf16 = torch.float16, torch.bfloat16
    if name.startswith("dense128"):       # N = 512: (N / 256) * chunks * S < 256 -> verify_gemm_kernel (128 x 128 tiles)
        dt = f16 if name.endswith("f16") and not name.endswith("bf16") else bf16
        return cached((name,), lambda: mk_dense(512, K_SMALL, dt, dev, 21)), dt, [(1, {}), (5, {}), (16, {})]
    if name.startswith("denseR"):         # N = 4096, S = 16: 16 * chunks * 16 >= 256 -> verify_gemm_r_kernel, 128- / 144-token items
        dt = bf16 if name.endswith("bf16") else f16
        return cached((name,), lambda: mk_dense(4096, K_SMALL, dt, dev, 22)), dt, [(16, {})]
    if name == "int4-128":                # fp16 int4 below vgemm.hip's workgroup floor -> verify_gemm_kernel<F16, 2>
        return cached(("wi4",), lambda: mk_int4(512, K_SMALL, dev, 23)), f16, [(1, {}), (5, {}), (16, {})]
    if name == "vgw":                     # UMB_VGW_MIN_WGS=1 (read per call): vgemm_w_kernel on the same small matrix
        e = {"UMB_VGW_MIN_WGS": "1"}
        return cached(("wi4",), lambda: mk_int4(512, K_SMALL, dev, 23)), f16, [(1, e), (3, e), (5, e), (7, e), (16, e)]
    if name == "vgw-k384":                # slabs of 2 + 1 k-blocks
        return cached(("wi4k384",), lambda: mk_int4(768, 384, dev, 24)), f16, [(2, {"UMB_VGW_MIN_WGS": "1"}), (3, {"UMB_VGW_MIN_WGS": "1"})]
    if name == "folded-bf16-chunks":      # bf16 int4 has no wide kernel: 64-row launches of the skinny kernel at row offsets
        return cached(("int4",), lambda: mk_int4(960, K_SMALL, dev, 12)), bf16, [(3, {}), (5, {})]
    raise KeyError(name)


WIDE = ["dense128-f16", "dense128-bf16", "denseR-f16", "denseR-bf16", "int4-128", "vgw", "vgw-k384", "folded-bf16-chunks"]


@gpu
@pytest.mark.parametrize("T", T_WIDE)
@pytest.mark.parametrize("name", WIDE)
def test_wide_every_slab_bit_for_bit(dev, name, T):
    o, dtype, runs = wide_case(dev, name)
    x64 = wide_x(dev, o.K)[:T]
    x = strided(x64, dtype)
    for S, e in runs:
        with env(**e):
            got = run_gemm(o, x, T, S, 1)
        assert_same_bits(got, slab_refs(x64, o.Wd, S), f"{name} T={T} S={S}")


@gpu
@pytest.mark.parametrize("T", [385, 400, 512])
def test_wide_register_kernel_empty_trailing_slab(dev, T):
    """verify_gemm_r_kernel (dense) with KB = 4, S = 3: slabs of 2, 2 and 0 k-blocks; N = 8192 so that 32 * chunks * 3 >= 256
    (385 / 400: three 144-token items, 512: four 128-token items)"""
    o = cached(("dense8192k512",), lambda: mk_dense(8192, 512, torch.float16, dev, 25))
    x64 = wide_x(dev, 512)[:T]
    got = run_gemm(o, strided(x64, torch.float16), T, 3, 1)
    assert float(got[2].abs().max()) == 0.0
    assert_same_bits(got, slab_refs(x64, o.Wd, 3), f"T={T}")


@gpu
def test_empty_slab_contract(dev):
    """include/umbrella_hip.h (umb_gemm): a split without k-blocks is written as zeros by every family; vgemm.hip's kernel,
    which leaves such a block at once, must not be offered the launch"""
    from umbrella_amd import _lib
    lib = _lib.load()
    with env(UMB_VGW_MIN_WGS="1"):
        assert lib.umb_vgemm_w_ok(130, 512, 2048, 3, 0) == 1 and lib.umb_vgemm_w_ok(130, 512, 2048, 6, 0) == 1
        for S in (5, 7, 9, 10, 11, 12, 13, 14, 15, 17):           # per = ceil(16 / S) leaves (S - 1) * per >= 16
            assert lib.umb_vgemm_w_ok(130, 512, 2048, S, 0) == 0, S
        o = cached(("wi4",), lambda: mk_int4(512, K_SMALL, dev, 23))
        for T, dtype in ((13, torch.float16), (13, torch.bfloat16), (130, torch.float16), (300, torch.float16)):
            x64 = wide_x(dev, K_SMALL)[:T]
            for S in (5, 7, 15, 17):
                got = run_gemm(o, strided(x64, dtype), T, S, 1)
                k0, k1 = slab_range(16, S, S - 1)
                assert k0 == k1 and float(got[S - 1].abs().max()) == 0.0, (T, S)
                assert_same_bits(got, slab_refs(x64, o.Wd, S), f"T={T} S={S} {dtype}")


# once-per-process settings: UMB_VGW=0 hands fp16 int4 at T > 64 to gemm.hip's kernels -- verify_gemm_pp_kernel (shared
# activation staging at an even row-block count, the token-chunk pairing at an odd one) and the int4 verify_gemm_r_kernel
# (odd row blocks x odd chunks)
def _child_vgw0():
    dev = torch.device("cuda:0")
    n = 0
    for N, Ts in ((4096, (256, 257, 385)), (3840, (256, 257, 384, 385))):
        o = mk_int4(N, K_SMALL, dev, 31 + N)
        for T in Ts:
            x64 = int_x(T, K_SMALL, dev, T)
            got = run_gemm(o, strided(x64, torch.float16), T, 16, 1)
            assert_same_bits(got, slab_refs(x64, o.Wd, 16), f"UMB_VGW=0 N={N} T={T}")
            n += 1
    print(f"child ok {n}")


@gpu
def test_wide_int4_kernels_behind_umb_vgw_0(dev):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "vgw0"], env=dict(os.environ, UMB_VGW="0"),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "child ok 7" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])


# ------------------------------------------------------------------ per-token 1/rms in the wide kernels' direct epilogues
def rms_fx(T, K, ms, dev):
    """UmbGemmFused whose ssq_in [T][RMS_STRIDE] makes 1/rms of row t exactly 2^-m_t (m_t cycling through ms): RMS_G valid groups
    of K * 4^m_t / RMS_G each, 1e9 behind them, ssq_dim = K, eps = 0.  Returns (fx, the buffer it points to, float64 factors)."""
    from umbrella_amd import _lib
    m = torch.tensor(ms, dtype=torch.float64, device=dev)[torch.arange(T, device=dev) % len(ms)]
    ssq = torch.full((T, RMS_STRIDE), 1e9, dtype=torch.float32, device=dev)
    ssq[:, :RMS_G] = (K * 4.0 ** m / RMS_G).float()[:, None]
    fx = _lib.UmbGemmFused()
    fx.ssq_in, fx.ssq_groups, fx.pad0, fx.ssq_dim, fx.eps = ssq.data_ptr(), RMS_G, RMS_STRIDE, float(K), 0.0
    return fx, ssq, 2.0 ** -m


def check_rms_round(o, x64, dtype, S, what, e=None):
    """epi 1: every slab is float64 product * 1/rms, a value of the model dtype, bit for bit"""
    T = x64.shape[0]
    fx, ssq, inv = rms_fx(T, o.K, RMS_M, x64.device)
    want64 = slab_refs(x64, o.Wd, S).double() * inv[None, :, None]
    want = want64.to(dtype)
    assert torch.equal(want.double(), want64), f"{what}: an expected value is not a {dtype} value"
    with env(**(e or {})):
        got = run_gemm(o, strided(x64, dtype), T, S, 1, epi=1, fx=fx)
    print(f"{what}: max |want| {float(want64.abs().max())}, differing values {int((got != want.float()).sum())}")
    assert_same_bits(got, want.float(), what)


def check_rms_silu(kind, dtype, T, dev, what, e=None):
    """epi 2 on one-hot rows: act[t, m] = gate * up * (1/rms)^2 with 1/rms in {2, 1} (gates 64 or 32: SiLU is the identity)"""
    I, K = 512, 512
    o, act64 = cached(("silu", kind, dtype if kind == "dense" else None), lambda: silu_weights(kind, dtype, I, K, dev))
    ks = probe_ks(K, (1,))
    ks = [ks[i % len(ks)] for i in range(T)]
    fx, ssq, inv = rms_fx(T, K, RMS_M[:2], dev)
    want64 = act64[torch.tensor(ks, device=dev)] * (inv * inv)[:, None]
    want = want64.to(dtype)
    assert torch.equal(want.double(), want64), f"{what}: an expected value is not a {dtype} value"
    act = torch.full((T, I), float("nan"), dtype=dtype, device=dev)
    with env(**(e or {})):
        run_gemm(o, strided(onehot(ks, K, dev), dtype), T, 1, 1, epi=2, fx=fx, out=act)
    print(f"{what}: max |want| {float(want64.abs().max())}, differing values {int((act != want).sum())}")
    assert_same_bits(act[None], want[None], what)


@gpu
@pytest.mark.parametrize("T", T_RMS)
@pytest.mark.parametrize("route", ["dense128-f16", "dense128-bf16", "denseR-f16", "denseR-bf16", "int4-128", "vgw"])
def test_wide_epilogues_apply_token_rms_exactly(dev, route, T):
    """The per-token 1/rms of the wide kernels' direct epilogues (fx.ssq_in; epi 1 and epi 2), S = 1: verify_gemm_kernel (dense
    and int4; N = 512 and N = 4096), vgemm_w_kernel, and the skinny kernel on the tail row of T = 129.  The true factors are
    2, 1, 0.5 and EVERY expected value is exactly representable in the output dtype (asserted here on the float64 expectations;
    magnitudes: test_token_rms_bounds), so a last-bit difference of the hardware rsqrtf (2^-23 relative) cannot carry a result
    across a rounding boundary: half a 16-bit ulp is at least 2^-12 relative.  At S = 1 these matrices stay below the 256
    work items verify_gemm_r_kernel wants, so the denseR routes also run their own split (S = 16), which reaches it; its int4
    instantiation and verify_gemm_pp_kernel sit behind UMB_VGW=0 (the child-process test below)."""
    o, dtype, runs = wide_case(dev, route)
    e = runs[0][1]
    if o.awq:                                                              # all scales 1.0: acc is an integer
        o = cached(("wi4s1",), lambda: mk_int4(512, K_SMALL, dev, 26, s=torch.ones(K_SMALL // 128, 512, device=dev).half()))
    x64 = cached(("xw-sparse", o.K), lambda: int_x(512, o.K, dev, 7 + o.K, nnz=SPARSE_NNZ))[:T]
    check_rms_round(o, x64, dtype, 1, f"{route} epi 1 T={T} S=1", e)
    if route.startswith("denseR"):
        check_rms_round(o, x64, dtype, runs[0][0], f"{route} epi 1 T={T} S={runs[0][0]}", e)
    check_rms_silu("int4" if o.awq else "dense", dtype, T, dev, f"{route} epi 2 T={T}", e)


def _child_vgw0_rms():
    dev = torch.device("cuda:0")
    n = 0
    for N, Ts in ((4096, (257, 385)), (3840, (257, 385))):
        o = mk_int4(N, K_SMALL, dev, 31 + N, s=torch.ones(K_SMALL // 128, N, device=dev).half())
        for T in Ts:
            check_rms_round(o, int_x(T, K_SMALL, dev, T, nnz=SPARSE_NNZ), torch.float16, 16, f"UMB_VGW=0 epi 1 N={N} T={T}")
            n += 1
    print(f"child ok {n}")


@gpu
def test_wide_int4_epilogues_behind_umb_vgw_0_apply_token_rms(dev):
    """epi 1 with the exact per-token factors on verify_gemm_pp_kernel (shared staging at N = 4096, the token-chunk pairing at
    N = 3840, T = 257) and the int4 verify_gemm_r_kernel (N = 3840, T = 385)"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "vgw0-rms"], env=dict(os.environ, UMB_VGW="0"),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "child ok 4" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])


# ------------------------------------------------------------------ one-hot probes: the weights read back element by element
def probe_ks(K, splits):
    """k positions: every residue mod 128 (spread over the k-blocks) and both edges of every slab of every split count used"""
    KB = K // 128
    ks = [r + 128 * ((r * 5) % KB) for r in range(128)]
    for S in splits:
        for s in range(S):
            k0, k1 = slab_range(KB, S, s)
            if k1 > k0:
                ks += [k0 * 128, k1 * 128 - 1]
    return sorted(set(ks))


def onehot(ks, K, dev):
    x = torch.zeros(len(ks), K, dtype=torch.float64, device=dev)
    x[torch.arange(len(ks), device=dev), torch.tensor(ks, device=dev)] = 1.0
    return x


def onehot_want(vals, ks, K, S):
    """vals [K, N] fp32: out[s, t] = vals[k_t] inside slab s, zeros elsewhere"""
    kt = torch.tensor(ks, device=vals.device)
    rows, zero = vals[kt], torch.zeros((), dtype=torch.float32, device=vals.device)
    out = torch.zeros(S, len(ks), vals.shape[1], dtype=torch.float32, device=vals.device)
    for s in range(S):
        k0, k1 = slab_range(K // 128, S, s)
        out[s] = torch.where(((kt >= k0 * 128) & (kt < k1 * 128))[:, None], rows, zero)
    return out


PROBE_S = (1, 3, 5, 16)


@gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_onehot_rows_read_every_weight_back(dev, form):
    """real (non power of two) scales.  exact form: fp32(fp16((q - z) * s)); folded form: fp32(s) * fp32(q - z); dense: W itself.
    epi 1 on the same rows: dense values are already 16-bit, so the rounding is the identity."""
    kind, dtype, dq = FORMS[form]
    N, K = (992, K_SMALL) if kind == "dense" else (960, K_SMALL)
    if kind == "dense":
        W = (torch.randn(N, K, device=dev, generator=_gen(dev, 41)) * 0.05).to(dtype)
        o = mk_dense(N, K, dtype, dev, 0, W=W.double())
        vals = W.float().t().contiguous()
    else:
        o = cached(("int4real",), lambda: mk_int4(N, K, dev, 42, real_scales=True))
        prod = o.d.float() * o.s.float()                                    # 4-bit x 11-bit: exact in fp32
        assert torch.equal(prod.double(), o.d * o.s)
        vals = prod.half().float() if dq else prod
    ks = probe_ks(K, PROBE_S)
    with env(UMB_DEQUANT=dq):
        for t0 in range(0, len(ks), 64):
            part = ks[t0:t0 + 64]                                          # full 64-row launches and a ragged last one
            x = strided(onehot(part, K, dev), dtype)
            for S in PROBE_S:
                want = onehot_want(vals, part, K, S)
                for Rtb in (1, VARIANTS["r2tb7"], VARIANTS["r1tb7w8"]):
                    assert_same_bits(run_gemm(o, x, len(part), S, Rtb), want, f"{form} rows {t0}.. S={S} Rtb={Rtb:#x}")
            if kind == "dense":
                assert_same_bits(run_gemm(o, x, len(part), 1, 1, epi=1), onehot_want(vals, part, K, 1), f"{form} epi 1 rows {t0}..")


@gpu
@pytest.mark.parametrize("route", ["int4-128", "vgw"])
def test_onehot_rows_wide_exact_dequant(dev, route):
    """T > 64: every one-hot row in ONE launch; W = fp16((q - z) * s) bit for bit on the 128 x 128 kernel and on vgemm.hip"""
    N, K = 512, K_SMALL
    o = cached(("int4real512",), lambda: mk_int4(N, K, dev, 43, real_scales=True))
    vals = (o.d.float() * o.s.float()).half().float()
    ks = probe_ks(K, (1, 3, 16))
    x = strided(onehot(ks, K, dev), torch.float16)
    assert len(ks) > 128
    with env(UMB_VGW_MIN_WGS="1" if route == "vgw" else None):
        for S in (1, 3, 16):
            assert_same_bits(run_gemm(o, x, len(ks), S, 1), onehot_want(vals, ks, K, S), f"{route} S={S}")


# ------------------------------------------------------------------ 3. SiLU(gate) * up on one-hot rows
def silu_weights(kind, dtype, I, K, dev):
    g = _gen(dev, 51)
    gate_on = torch.randint(0, 2, (K, I), device=dev, generator=g)
    up = torch.randint(-3, 4, (K, I), device=dev, generator=g)
    if kind == "dense":
        W = torch.cat([gate_on.double() * GATE_ON, up.double()], 1).t().contiguous()      # [2I, K], HF [gate; up] stack
        return mk_dense(2 * I, K, dtype, dev, 0, il=True, W=W), gate_on.double() * GATE_ON * up.double()
    # int4: gate = (8 q' - 0) * 4 with q' in {0, 1}; up = (q - 8) * 1 with q in 5 .. 11
    q = torch.cat([gate_on * 8, up + 8], 1).to(torch.uint8)
    z = torch.cat([torch.zeros(K // 128, I, device=dev), torch.full((K // 128, I), 8.0, device=dev)], 1).to(torch.uint8)
    s = torch.cat([torch.full((K // 128, I), 4.0, device=dev), torch.ones(K // 128, I, device=dev)], 1).half()
    return mk_int4(2 * I, K, dev, 0, il=True, q=q, z=z, s=s), gate_on.double() * GATE_ON * up.double()


@gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_silu_epilogue_onehot_exact(dev, form):
    """epi 2 and the gate / up interleave of umb_repack_dense / umb_awq_repack mode 1, row by row: act[t, m] = gate[m, k_t] *
    up[m, k_t] exactly (gates 0 or 32: SiLU is the identity there, test_silu_is_the_identity_on_the_gate_set), T <= 64 on the
    skinny kernel (row-major and FM in / out) and T > 64 on the wide kernels (fp16 int4: also vgemm.hip)"""
    from umbrella_amd import _lib
    from umbrella_amd.models.llama import from_fm, to_fm
    kind, dtype, dq = FORMS[form]
    I, K = 512, 512
    o, act64 = silu_weights(kind, dtype, I, K, dev)                        # act64 [K, I]
    assert o.lin.interleaved
    ks = probe_ks(K, (1,))
    with env(UMB_DEQUANT=dq):
        for t0 in range(0, len(ks), 64):
            part = ks[t0:t0 + 64]
            T = len(part)
            want = act64[torch.tensor(part, device=dev)].to(dtype)
            x = onehot(part, K, dev).to(dtype)
            for Rtb in (1, 2, VARIANTS["r1tb7w8"]):
                act = torch.full((T, I), float("nan"), dtype=dtype, device=dev)
                run_gemm(o, strided(x.double(), dtype), T, 1, Rtb, epi=2, out=act)
                assert_same_bits(act[None], want[None], f"{form} SiLU rows {t0}.. Rtb={Rtb:#x}")
            fx = _lib.UmbGemmFused()
            fx.pad1 = 3                                                    # FM in, FM out
            tt = _lib.load().umb_ll_token_tiles(T)
            act_fm = torch.zeros(tt * 16 * I, dtype=dtype, device=dev)
            run_gemm(o, to_fm(x), T, 1, 1, epi=2, fx=fx, out=act_fm)
            assert_same_bits(from_fm(act_fm, T, I)[None], want[None], f"{form} SiLU FM rows {t0}..")
        if dtype == torch.float16 or kind == "dense":
            T = len(ks)                                                    # > 64 rows: one wide launch
            want = act64[torch.tensor(ks, device=dev)].to(dtype)
            for e in ({}, {"UMB_VGW_MIN_WGS": "1"}):
                with env(**e):
                    act = torch.full((T, I), float("nan"), dtype=dtype, device=dev)
                    run_gemm(o, strided(onehot(ks, K, dev), dtype), T, 1, 1, epi=2, out=act)
                assert_same_bits(act[None], want[None], f"{form} SiLU wide {e}")


# ------------------------------------------------------------------ 4. the four families on the same operands
@gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("family", ["skinny", "skinny-round", "lowlat", "lowlat-round", "lowlat-int4", "gemv", "head-stream", "head-stream-fm"])
def test_all_families_agree_exactly(dev, family, dtype):
    """split-K MFMA kernel, whole-K low-latency kernel, row-streaming GEMV (residual epilogue on h = 0: h <- round(x W^T)) and the
    streamed head (1/rms = 1: 2048 / 2048 + 0) on the same sparse integer operands: one reference, the same bits"""
    from umbrella_amd import _lib
    lib = _lib.load()
    H = 2048
    N = 8208 if family.startswith("head") else 512
    x64 = cached(("xsparse",), lambda: int_x(64, H, dev, 61, nnz=SPARSE_NNZ))
    if family == "lowlat-int4":
        o = cached(("ll-int4",), lambda: mk_int4(512, H, dev, 62))
    else:
        o = cached(("fam", N, dtype), lambda: mk_dense(N, H, dtype, dev, 63 + N))
    ref = (x64 @ o.Wd).float()
    dt = _lib.dtype_code(dtype)
    if family.startswith("skinny"):
        for T in (1, 4, 8, 13, 40, 64):
            got = run_gemm(o, strided(x64[:T], dtype), T, 4, 1, epi=int(family.endswith("round")))
            want = slab_refs(x64[:T], o.Wd, 4)
            assert_same_bits(got, want, f"{family} T={T}")
            assert_same_bits(got.sum(0)[None], ref[None, :T].contiguous(), f"{family} T={T} summed")
    elif family.startswith("lowlat"):
        for T in (1, 4, 8, 13, 40, 64):
            got = o.lin.apply_ll(x64[:T].to(dtype).contiguous(), round_out=family.endswith("round"))
            assert_same_bits(got[None], ref[None, :T].contiguous(), f"{family} T={T}")
    elif family == "gemv":
        rows = torch.empty_like(o.rows)
        _lib.call("umb_repack_rows", rows, o.rows, N, H, 0, 0, 0)
        for T in (1, 2, 3, 4):
            assert lib.umb_gemv_ok(T, N, H, 4) == 1
            groups = lib.umb_gemv_groups(T, N, H)
            h, hw = torch.zeros(T, N, dtype=dtype, device=dev), torch.zeros(T, N, dtype=dtype, device=dev)
            nw, ssq = torch.ones(N, dtype=dtype, device=dev), torch.zeros(T, groups, device=dev)
            fx = _lib.UmbGemmLL()
            fx.h, fx.hw, fx.norm_w, fx.ssq_out, fx.ssq_out_stride = h.data_ptr(), hw.data_ptr(), nw.data_ptr(), ssq.data_ptr(), groups
            _lib.call("umb_gemv", None, x64[:T].to(dtype).contiguous(), rows, T, N, H, 4, fx, dt)
            assert_same_bits(h.float()[None], ref[None, :T].contiguous(), f"gemv T={T}")
            assert_same_bits(hw[None], h[None], f"gemv hw T={T}")
            assert_same_bits(ssq.sum(1)[None, None], ref[:T].pow(2).sum(1)[None, None], f"gemv ssq T={T}")   # integers < 2^24: exact
    else:
        fm = family.endswith("fm")
        G, stride = 32, 32
        for rows in (1, 3, 5, 8):
            assert lib.umb_head_stream_ok(rows, N, H) == 1
            ssq = torch.full((rows, stride), float(H // G), device=dev)
            x = x64[:rows].to(dtype).contiguous()
            if fm:
                xin = torch.zeros(16 * H, dtype=dtype, device=dev)
                _lib.call("umb_to_fm", xin, x, rows, H, dt)
                x = xin
            out = torch.full((rows, N), float("nan"), device=dev)
            _lib.call("umb_head_stream", out, x, ssq, stride, G, 0.0, o.rows, rows, N, H, 1 if fm else 0, dt)
            assert_same_bits(out[None], ref[None, :rows].contiguous(), f"{family} rows={rows}")


# ------------------------------------------------------------------ 5. the plan variants that exist only at full size
@gpu
@pytest.mark.parametrize("case", ["70b-gu-int4-tb7", "70b-gu-int4-tb14w8", "8b-gu-int4-w8", "8b-gu-bf16-w8"])
def test_full_size_plan_variants_every_column(dev, case):
    """70B gate/up (57344 x 8192: 4-wave blocks of 7 tiles split in two, one 8-wave block of 14 per CU unsplit) and 8B gate/up
    (28672 x 4096: one 8-wave block of 7 single tiles per CU) under the plan's own R / S / tb, T = 13, integer operands,
    EVERY column of every slab against float64 on the device"""
    N, K = (57344, 8192) if case.startswith("70b") else (28672, 4096)
    il = case != "70b-gu-int4-tb7"
    dtype = torch.bfloat16 if "bf16" in case else torch.float16
    o = mk_int4(N, K, dev, 71, il=il) if "int4" in case else mk_dense(N, K, dtype, dev, 72, il=il)
    lin = o.lin
    want_tb = {"70b-gu-int4-tb7": 7, "70b-gu-int4-tb14w8": 14 | 0x80}.get(case, 7 | 0x80)
    assert lin.tb == want_tb and lin.S == (1 if il else 2), (lin.R, lin.S, lin.tb)
    x64 = int_x(13, K, dev, 73)
    got = run_gemm(o, strided(x64, dtype), 13, lin.S, lin.Rtb)
    KB = K // 128
    for s in range(lin.S):
        k0, k1 = slab_range(KB, lin.S, s)
        for c0 in range(0, N, 8192):                                      # float64 chunks
            want = (x64[:, k0 * 128:k1 * 128] @ o.Wd[k0 * 128:k1 * 128, c0:c0 + 8192])
            w32 = want.float()
            assert torch.equal(w32.double(), want)
            assert_same_bits(got[s:s + 1, :, c0:c0 + 8192], w32[None], f"{case} split {s} columns {c0}..")


# ------------------------------------------------------------------ 6. CPU: a model GEMM with one seeded defect each
DEFECTS = ["kblock_in_neighbouring_split", "ragged_slab_last_kblock_dropped", "two_ntiles_swapped", "zero_point_from_next_column",
           "nibbles_swapped_in_one_tile", "last_row_of_token_tile_duplicated", "sum_x_correction_missing_for_one_kblock"]


def model_gemm(x, q, z, s, S, defect=None):
    """tiled split-K int4 GEMM in the folded form, float64: out[S, T, N]; tiles 16 columns x 128 k, blocks of 4 tiles"""
    T, K = x.shape
    N = q.shape[1]
    KB = K // 128
    out = np.zeros((S, T, N))
    q = q.astype(np.float64).copy()
    z = z.astype(np.float64).copy()
    if defect == "zero_point_from_next_column":
        c = next(c for c in range(N - 1) if np.any(z[:, c] != z[:, c + 1]))
        z[:, c] = z[:, c + 1]
    if defect == "nibbles_swapped_in_one_tile":
        blk = q[128:256, 16:32].copy()
        q[128:256:2, 16:32], q[129:256:2, 16:32] = blk[1::2], blk[0::2]
    for sp in range(S):
        k0, k1 = slab_range(KB, S, sp)
        for kb in range(k0, k1):
            dst = sp
            if defect == "kblock_in_neighbouring_split" and sp == 0 and kb == k1 - 1 and S > 1:
                dst = 1
            if defect == "ragged_slab_last_kblock_dropped" and sp == S - 1 and kb == k1 - 1:
                continue
            xs = x[:, kb * 128:(kb + 1) * 128]
            sx = xs.sum(1, keepdims=True)
            ga = xs @ q[kb * 128:(kb + 1) * 128]
            corr = z[kb][None] * sx
            if defect == "sum_x_correction_missing_for_one_kblock" and kb == 1:
                corr[:, 32:48] = 0
            out[dst] += s[kb][None].astype(np.float64) * (ga - corr)
    if defect == "two_ntiles_swapped":
        out[:, :, 64:80], out[:, :, 80:96] = out[:, :, 80:96].copy(), out[:, :, 64:80].copy()
    if defect == "last_row_of_token_tile_duplicated":
        out[:, T - 1] = out[:, T - 2]
    return out


def _model_operands(exact, T=13, N=256, K=2048, seed=3):
    rs = np.random.RandomState(seed)
    q = rs.randint(0, 16, size=(K, N))
    z = rs.randint(0, 16, size=(K // 128, N))
    if exact:
        s = 2.0 ** rs.choice(SCALE_EXPS, size=(K // 128, N))
        x = rs.randint(-XA, XA + 1, size=(T, K)).astype(np.float64)
    else:                                         # test_gemm_awq's operands
        s = (rs.rand(K // 128, N) * 0.02 + 0.002).astype(np.float16).astype(np.float64)
        x = torch.from_numpy(rs.randn(T, K).astype(np.float32)).half().double().numpy()
    return x, q, z, s


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_seeded_defect_fails_the_exact_comparison(defect):
    x, q, z, s = _model_operands(True)
    S = 3                                          # KB = 16: slabs of 6, 6 and 4 k-blocks
    want = torch.from_numpy(model_gemm(x, q, z, s, S)).float()
    assert_same_bits(torch.from_numpy(model_gemm(x, q, z, s, S)).float(), want, "the model against itself")
    with pytest.raises(AssertionError, match="values differ"):
        assert_same_bits(torch.from_numpy(model_gemm(x, q, z, s, S, defect)).float(), want, defect)
    # an unwritten (NaN) slab is a difference too
    nanbuf = want.clone()
    nanbuf[2] = float("nan")
    with pytest.raises(AssertionError, match="values differ"):
        assert_same_bits(nanbuf, want, "unwritten slab")


def test_which_defects_the_relative_metric_lets_through():
    """the record of what the exact tests add: `max|a - b| / max|b| < 2e-3` on the summed partials, test_gemm_awq's data.
    Printed, not asserted."""
    x, q, z, s = _model_operands(False)
    ref = model_gemm(x, q, z, s, 1)[0]
    passed = []
    for d in DEFECTS:
        out = model_gemm(x, q, z, s, 3, d).sum(0)
        rel = float(np.abs(out - ref).max() / (np.abs(ref).max() + 1e-9))
        print(f"defect {d}: rel {rel:.3e} -> {'PASSES' if rel < 2e-3 else 'fails'} the 2e-3 metric")
        if rel < 2e-3:
            passed.append(d)
    print("defects the relative metric lets through:", passed)
    try:
        from conftest import report_fact
        report_fact("gemm_exact.defects_the_relative_metric_passes", passed)
    except ImportError:
        pass


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    {"vgw0": _child_vgw0, "vgw0-rms": _child_vgw0_rms}[sys.argv[1]]()
