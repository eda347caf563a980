"""Every kernel family that finishes a q/k/v projection or a residual add writes the same bytes (csrc/qkv_epilogue.h).

The rotation, the head routing, the KV append and the 4-wide residual step live once, in csrc/qkv_epilogue.h; seven kernels call
them.  This module feeds ONE set of operands to every family and compares each family's whole output buffers, bit for bit, with
the host reference of tests/test_lowlat_exact.py (model_qkv / cache_expected / model_resid; builders and comparisons are imported
from there and from tests/test_gemm_exact.py, nothing is restated here).  No tolerance appears below.

q/k/v families
  fused S=1   umb_gemm_fused epi 3, one block per n-group runs the epilogue            (gemm.hip skinny_gemm_kernel)
  fused S=2   umb_gemm_fused epi 3, the last of two split blocks sums and finishes      (the same kernel's last-arriver path)
  split       umb_gemm (S = 2 fp32 partials) + umb_reduce_qkv_rope2                    (epilogue.hip reduce_qkv_rope_kernel)
  lowlat      umb_gemm_ll epi 3                                                         (lowlat.hip ll_gemm_kernel)
  gemv        umb_gemv epi 3, T <= 4                                                    (gemv.hip gv_kernel)
each with and without the per-token 1/rms; split, lowlat and gemv also with and without a projection bias (the fused epilogue of
gemm.hip has none).  The persistent chain is tied to the GEMV launches by tests/test_chain.py.

Operands (regime B of test_lowlat_exact.py, at this module's shapes).  x: NNZ integers of |x| <= 3 per row, W: integers of
|W| <= 3, K = 256: every partial sum in any order is an integer below 2^24, so the MFMA chains, the split sums, the LDS slice sums
and the v_dot2 chains + butterflies all hold the float64 matmul.  The producer's sums of squares are c_g * 4^m_t in 8 groups (row
stride 12, NaN behind the groups), m_t in {-1, 0}: 1/rms is 2 or 1; the bias is a small integer; so the value in front of RoPE is
an integer below 2^8 (asserted on the float64 expectation) and a last-bit error of the hardware rsqrt cannot move it.  cos / sin
are arbitrary 16-bit values: every product of the rotation is a real rounding.  The weight rows of features 0 .. 15 and their
partners in q head 1 and k head 1 are zero (and so is their bias): their products are +-0 by the sign of cos / sin, and the
sign bit of the result is compared like every other bit (the expectation is asserted to contain -0 in q and in K).

The GEMV family needs K = 2048: it runs on the same operands with x and W padded by zero columns (exact zeros add nothing).

Residual: umb_gemm_fused epi 4 (S = 1, 2), umb_gemm_ll epi 4 and umb_gemv epi 4 (T <= 4) on integer h0 and the same sparse
operands: h, hw (row-major; the low-latency FM buffer through umb_from_fm) and every sums-of-squares group (an integer below
2^24, compared with the float64 sum over the reference h -- equal groups give equal per-token totals).
"""
import pytest
import torch

from test_gemm_exact import cached, dev, int_x  # noqa: F401  (dev: the module-scoped device fixture)
from test_lowlat_exact import (DTYPES, NAN, RMS_M_QKV, SENT, _fx, _plan, cache_expected, exact32, gemv, group_ssq, gv_rows, model_inv,
                               model_qkv, model_resid, pack, pick_pos_slot, qkv_tables, rnd, same, sent, ssq_rows, tt_of)
from umbrella_amd.attn.cache import VT_PAD

gpu = pytest.mark.gpu

HQ, HKV, LMAX, K, K_GV = 4, 2, 64, 256, 2048
T_ALL = (1, 3, 17)                     # 17: the second token tile and idle lanes; the GEMV family takes T <= 4
NNZ = 5                                # |acc| <= 5 * 9, times 1/rms <= 2, plus |bias| <= 3: an integer below 2^8
G, G_STRIDE = 8, 12                    # sums-of-squares groups / row stride (umb_gemm_fused reads them four at a time)
ZERO_HEADS, ZERO_M = (1, HQ + 1), 16   # heads (of the [q | k | v] stack) whose features 0 .. 15 and partners have zero weights


def test_bounds():
    assert NNZ * 3 * 3 * max(2.0 ** -m for m in RMS_M_QKV) + 3 < 2 ** 8 and K * 9 < 2 ** 24
    assert G % 4 == 0 and G_STRIDE % 4 == 0 and G_STRIDE > G


def zero_features(D):
    """HF feature indices (columns of the [q | k | v] output) whose weight rows are zero: (m, m + D/2) pairs of two heads"""
    m = torch.arange(ZERO_M)
    return torch.cat([h * D + torch.cat([m, m + D // 2]) for h in ZERO_HEADS])


def operands(D, dtype, dev):
    """(packed linear with RoPE partner rows, GEMV rows [N, 2048], x [17, 256] float64, acc [17, N] fp32 on the CPU)"""
    N = (HQ + 2 * HKV) * D

    def make():
        g = torch.Generator(device=dev).manual_seed(4100 + D)
        W = torch.randint(-3, 4, (N, K), device=dev, generator=g).double()
        W[zero_features(D).to(dev)] = 0.0
        o = pack("dense", W, W.t().contiguous(), dtype, mode=(D, HQ + HKV))
        Wpad = torch.cat([W, torch.zeros(N, K_GV - K, device=dev, dtype=W.dtype)], 1)
        o.gv_rows = gv_rows(Wpad.to(dtype), 2, D, HQ + HKV)
        x = int_x(max(T_ALL), K, dev, 4200 + D, nnz=NNZ)
        o.x, o.acc = x, exact32(x @ o.Wd).cpu()
        return o
    return cached(("qkve", D, dtype), make)


def rms_rows(T, dev):
    """(ssq [T, G_STRIDE] on the device with NaN behind the G groups, 1/rms [T] float64: 2 or 1)"""
    ssq, _ = ssq_rows(T, G, RMS_M_QKV)
    wide = torch.full((T, G_STRIDE), NAN, dtype=torch.float32)
    wide[:, :G] = ssq[:, :G]
    return wide.to(dev), model_inv(ssq, G)


class Bufs:
    """sentinel-filled q (one row more than T), K and V^T storage"""

    def __init__(self, T, D, dtype, dev):
        self.q, self.k = sent((T + 1, HQ, D), dtype, dev), sent((HKV, LMAX, D), dtype, dev)
        self.vt = sent((HKV, D, LMAX + VT_PAD), dtype, dev)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", T_ALL)
@pytest.mark.parametrize("D", [64, 128])
def test_every_qkv_family_writes_the_reference_bytes(dev, D, T, dtype):
    from umbrella_amd import _lib
    N, dt = (HQ + 2 * HKV) * D, _lib.dtype_code(dtype)
    o = operands(D, dtype, dev)
    cos, sin, _, bias = qkv_tables(N, D, dtype, 4300 + D)
    bias[zero_features(D)] = 0.0
    pos, slot = pick_pos_slot(T, cos.shape[0], LMAX, T + D)
    assert not torch.equal(pos, torch.arange(T, dtype=torch.int32)) and not torch.equal(slot, torch.arange(T, dtype=torch.int32))
    posd, slotd, cosd, sind, biasd = pos.to(dev), slot.to(dev), cos.to(dev), sin.to(dev), bias.to(dev)
    ssq, inv = rms_rows(T, dev)
    x16 = o.x[:T].to(dtype).contiguous()
    xpad = torch.cat([x16, torch.zeros(T, K_GV - K, dtype=dtype, device=dev)], 1).contiguous()
    counters = torch.zeros(64, dtype=torch.int32, device=dev)
    neg_zero = 0

    for use_rms in (False, True):
        for use_bias in (False, True):
            b, iv = (bias if use_bias else None), (inv if use_rms else None)
            y = o.acc[:T].double() * (iv[:, None] if use_rms else 1.0) + (b.double()[None] if use_bias else 0.0)
            assert torch.equal(rnd(y.float(), dtype).double(), y) and float(y.abs().max()) < 2 ** 8
            q, k, v = model_qkv(o.acc[:T], dtype, pos, cos, sin, HQ, HKV, D, inv=iv, bias=b)
            wq = torch.cat([q, torch.full((1, HQ, D), SENT, dtype=dtype)])
            wk, wv = cache_expected(k, v, slot, LMAX)
            if not use_bias:
                nq, nk = int((q.view(torch.int16) == -32768).sum()), int((k.view(torch.int16) == -32768).sum())
                assert nq > 0 and nk > 0, "the zero rows give no -0 in the expectation"
                neg_zero += nq + nk
            rkw = dict(ssq_in=ssq, ssq_groups=G, ssq_dim=float(1024), eps=0.0) if use_rms else {}
            tag = f"D={D} T={T} {dtype} rms={use_rms} bias={use_bias}"

            def check(bf, family):
                same(bf.q, wq, f"{family} {tag} q_out")
                same(bf.k, wk, f"{family} {tag} K storage")
                same(bf.vt, wv, f"{family} {tag} V^T storage")

            def dest(bf):
                return dict(pos=posd, slot=slotd, cosT=cosd, sinT=sind, q_out=bf.q, k_cache=bf.k, vt_cache=bf.vt, Hq=HQ, Hkv=HKV,
                            D=D, Lmax=LMAX)

            if not use_bias:
                for S in (1, 2):                                             # umb_gemm_fused epi 3: no bias in this epilogue
                    bf = Bufs(T, D, dtype, dev)
                    part = torch.full((S * T * N + 64,), NAN, dtype=torch.float32, device=dev)
                    fx = _fx(_lib.UmbGemmFused, counters=counters, pad0=G_STRIDE if use_rms else 0, **dest(bf), **rkw)
                    _lib.call("umb_gemm_fused", part, x16, K, o.lin.w, o.lin.meta, T, N, K, 0, S, 1, 3, fx, dt)
                    check(bf, f"fused S={S}")
                    assert int(counters.abs().sum()) == 0
            # split path: fp32 partials of two K slabs, then the reduce kernel
            bf = Bufs(T, D, dtype, dev)
            part = torch.full((2, T, N), NAN, dtype=torch.float32, device=dev)
            _lib.call("umb_gemm", part, x16, K, o.lin.w, o.lin.meta, T, N, K, 0, 2, 1, 0, dt)
            _lib.call("umb_reduce_qkv_rope2", part, 2, T, HQ, HKV, D, LMAX, posd, slotd, cosd, sind, bf.q, bf.k, bf.vt, 1,
                      biasd if use_bias else None, ssq if use_rms else None, G if use_rms else 0, G_STRIDE if use_rms else 0,
                      1024.0 if use_rms else 0.0, 0.0, dt)
            check(bf, "split + reduce")
            # low-latency and GEMV launches share the argument struct
            llkw = dict(rkw, ssq_in_stride=G_STRIDE) if use_rms else {}
            bf = Bufs(T, D, dtype, dev)
            o.lin.apply_ll(x16, fx=_fx(bias=biasd if use_bias else None, **dest(bf), **llkw), epi=3)
            check(bf, "lowlat")
            if T <= 4:
                bf = Bufs(T, D, dtype, dev)
                gemv(None, xpad, o.gv_rows, T, N, K_GV, 3, _fx(bias=biasd if use_bias else None, **dest(bf), **llkw))
                check(bf, "gemv")
    assert neg_zero > 0


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", T_ALL)
def test_every_residual_family_writes_the_reference_bytes(dev, T, dtype):
    from umbrella_amd import _lib
    from umbrella_amd.models.llama import from_fm
    N, dt = 512, _lib.dtype_code(dtype)

    def make():
        g = torch.Generator(device=dev).manual_seed(4400)
        W = torch.randint(-3, 4, (N, K), device=dev, generator=g).double()
        o = pack("dense", W, W.t().contiguous(), dtype)
        o.gv_rows = gv_rows(torch.cat([W, torch.zeros(N, K_GV - K, device=dev, dtype=W.dtype)], 1).to(dtype))
        o.x = int_x(max(T_ALL), K, dev, 4500, nnz=NNZ)
        o.acc = exact32(o.x @ o.Wd).cpu()
        return o
    o = cached(("qkve-resid", dtype), make)
    g = torch.Generator().manual_seed(4600)
    nw = (1 + 0.1 * torch.randn(N, generator=g)).to(dtype)
    h0 = torch.randint(-3, 4, (max(T_ALL), N), generator=g).to(dtype)[:T]
    wh, whw = model_resid(o.acc[:T], h0, nw, dtype)
    assert torch.equal(wh.double(), o.acc[:T].double() + h0.double())
    x16, nwd = o.x[:T].to(dtype).contiguous(), nw.to(dev)
    pad = 3                                                                  # untouched columns behind the groups of every family

    def want_ssq(groups):
        w = torch.full((T, groups + pad), -1.0)
        w[:, :groups] = group_ssq(wh, N // groups)
        return w

    counters = torch.zeros(64, dtype=torch.int32, device=dev)
    for S in (1, 2):
        h, hw, ssq = h0.to(dev), sent((T, N), dtype, dev), torch.full((T, N // 64 + pad), -1.0, device=dev)
        part = torch.full((S * T * N + 64,), NAN, dtype=torch.float32, device=dev)
        fx = _fx(_lib.UmbGemmFused, counters=counters, h=h, hw=hw, norm_w=nwd, ssq_out=ssq, ssq_out_stride=N // 64 + pad)
        _lib.call("umb_gemm_fused", part, x16, K, o.lin.w, o.lin.meta, T, N, K, 0, S, 1, 4, fx, dt)
        same(h, wh, f"fused S={S} T={T} h")
        same(hw, whw, f"fused S={S} T={T} hw")
        same(ssq, want_ssq(N // 64), f"fused S={S} T={T} ssq_out")
        assert int(counters.abs().sum()) == 0
    groups = N // 16 // _plan(N, K, False)[0]
    h, hw, ssq = h0.to(dev), sent((tt_of(T) * 16 * N,), dtype, dev), torch.full((T, groups + pad), -1.0, device=dev)
    o.lin.apply_ll(x16, fx=_fx(h=h, hw=hw, norm_w=nwd, ssq_out=ssq, ssq_out_stride=groups + pad), epi=4)
    same(h, wh, f"lowlat T={T} h")
    same(from_fm(hw, T, N), whw, f"lowlat T={T} hw")
    same(ssq, want_ssq(groups), f"lowlat T={T} ssq_out")
    if T <= 4:
        groups = _lib.load().umb_gemv_groups(T, N, K_GV)
        xpad = torch.cat([x16, torch.zeros(T, K_GV - K, dtype=dtype, device=dev)], 1).contiguous()
        h, hw, ssq = h0.to(dev), sent((T, N), dtype, dev), torch.full((T, groups + pad), -1.0, device=dev)
        gemv(None, xpad, o.gv_rows, T, N, K_GV, 4, _fx(h=h, hw=hw, norm_w=nwd, ssq_out=ssq, ssq_out_stride=groups + pad))
        same(h, wh, f"gemv T={T} h")
        same(hw, whw, f"gemv T={T} hw")
        same(ssq, want_ssq(groups), f"gemv T={T} ssq_out")
