"""Qwen3 dense models (0.6B ... 32B, per-head q/k RMSNorm) on the HIP path: config and registry, the CPU restatement
against HF's recorded logits, the proof that the fixture cannot be met without the head norms, and on the GPU the new
split-K reduce + head norm + RoPE + KV append kernel, the whole model against the fixture (dense, AWQ, offloaded, graph
replay), the deferred-norm and in-place schedules at published widths and both engines with a Qwen3 target and draft.

Fixture: tests/golden/make_golden_qwen3.py (HF Qwen3ForCausalLM, fp32, eager).  GPU tests read the fixture and
tests/qwen3_ref.py only."""
import dataclasses
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import qwen3_ref as qr
from helpers import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(GOLD, "qwen3.json")) as f:
    G = json.load(f)
LOG = np.load(os.path.join(GOLD, "qwen3_logits.npz"))
with open(os.path.join(GOLD, "growmaps.json")) as f:
    GM = json.load(f)
DTYPES = [torch.float16, torch.bfloat16]
IDS = [f"Qwen/Qwen3-{s}" for s in ("0.6B", "1.7B", "4B", "8B", "14B", "32B")] + \
      [f"Qwen/Qwen3-{s}-AWQ" for s in ("4B", "8B", "14B", "32B")]
LOGIT_TOL = {torch.float16: (0.06, 2.0 ** -9), torch.bfloat16: (0.35, 2.0 ** -6)}      # test_gemma2_logits_vs_fixture


def _tol_scale(ref) -> float:
    return max(1.0, float(np.abs(np.asarray(ref)).max()) / 16.0)


# ----------------------------------------------------------------------------- CPU
def test_qwen3_registry_traits():
    from umbrella_amd.models.auto_model import AutoModelLM
    from umbrella_amd.models.config import KNOWN
    from umbrella_amd.models.qwen3 import Qwen3
    dims = {"0.6B": (1024, 3072, 28, 16, 8, True), "1.7B": (2048, 6144, 28, 16, 8, True), "4B": (2560, 9728, 36, 32, 8, True),
            "8B": (4096, 12288, 36, 32, 8, False), "14B": (5120, 17408, 40, 40, 8, False), "32B": (5120, 25600, 64, 64, 8, False)}
    assert len(IDS) == 10
    for name in IDS:
        c = KNOWN[name]
        size = name.split("-")[1]
        assert (c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads,
                c.tie_word_embeddings) == dims[size], name
        assert c.family == "qwen3" and c.head_dim == 128 and c.vocab_size == 151936 and not c.attention_bias
        assert (c.rms_norm_eps, c.rope_theta, c.rope_scaling, c.max_position_embeddings) == (1e-6, 1e6, None, 40960)
        assert c.eos_token_id == [151645, 151643] and c.awq == name.endswith("-AWQ") and c.awq_group == 128
        for table in (AutoModelLM._MODEL_MAPPING, AutoModelLM._OFFLOAD_MODEL_MAPPING, AutoModelLM._CUDAGRAPH_MODEL_MAPPING):
            assert table[name] is Qwen3
    c = KNOWN["Qwen/Qwen3-0.6B"]
    assert c.q_dim == 2048 != c.hidden_size
    m = AutoModelLM.from_pretrained("Qwen/Qwen3-32B-AWQ", max_length=64)
    assert isinstance(m, Qwen3) and m.sched == "split" and not m.fused
    # every other family keeps its class and its defaults
    from umbrella_amd.models.llama import Llama
    assert AutoModelLM._MODEL_MAPPING["Qwen/Qwen2.5-7B-Instruct"] is Llama
    assert KNOWN["Qwen/Qwen2.5-7B-Instruct"].family == "llama"


def test_qwen3_from_dir(tmp_path):
    from umbrella_amd.models.auto_model import _dir_class
    from umbrella_amd.models.config import LlamaCfg
    from umbrella_amd.models.qwen3 import Qwen3
    cfg = {"model_type": "qwen3", "vocab_size": 151936, "hidden_size": 1024, "intermediate_size": 3072,
           "num_hidden_layers": 28, "num_attention_heads": 16, "num_key_value_heads": 8, "head_dim": 128, "rms_norm_eps": 1e-6,
           "rope_theta": 1000000, "rope_scaling": None, "max_position_embeddings": 40960, "tie_word_embeddings": True,
           "attention_bias": False, "use_sliding_window": False, "sliding_window": None, "max_window_layers": 28,
           "eos_token_id": 151645}
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    (tmp_path / "generation_config.json").write_text(json.dumps({"eos_token_id": [151645, 151643]}))
    c = LlamaCfg.from_dir(str(tmp_path))
    assert c.family == "qwen3" and c.head_dim == 128 and c.q_dim == 2048 and c.tie_word_embeddings and not c.attention_bias
    assert c.eos_token_id == [151645, 151643] and c.rope_theta == 1e6 and not c.awq and c.vocab_size == 151936
    assert _dir_class(str(tmp_path)) is Qwen3
    (tmp_path / "config.json").write_text(json.dumps(dict(cfg, layer_types=["full_attention"] * 28, attention_bias=True,
                                                          quantization_config={"quant_method": "awq", "group_size": 128})))
    c = LlamaCfg.from_dir(str(tmp_path))
    assert c.family == "qwen3" and c.attention_bias and c.awq
    for bad in (dict(cfg, layer_types=["full_attention"] * 27 + ["sliding_attention"]), dict(cfg, use_sliding_window=True),
                dict(cfg, model_type="qwen3_moe")):
        (tmp_path / "config.json").write_text(json.dumps(bad))
        with pytest.raises(NotImplementedError):
            LlamaCfg.from_dir(str(tmp_path))


def test_qwen3_config_never_reaches_the_llama_runtime():
    """plain Llama, the tensor-parallel and the layer-pipelined builders would skip the head norms on a Qwen3 config and emit
    plausible garbage: each refuses it before touching a device or a process group; Qwen3 refuses Llama configs"""
    from umbrella_amd.models.config import KNOWN
    from umbrella_amd.models.llama import Llama
    from umbrella_amd.models.qwen3 import Qwen3
    from umbrella_amd.parallel import build_pipelined_engine
    from umbrella_amd.tensor_parallel import TensorParallelLlama, build_tp_engine
    name = "Qwen/Qwen3-32B-AWQ"
    with pytest.raises(NotImplementedError, match="qwen3"):
        Llama(name)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        TensorParallelLlama.build(KNOWN[name], {}, None, 256, "cpu", torch.bfloat16)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        build_tp_engine("cpu", model=name, draft_model="Qwen/Qwen3-0.6B", engine="static")
    with pytest.raises(NotImplementedError, match="layer pipelining"):
        build_pipelined_engine("cpu", model=name, draft_model="Qwen/Qwen3-0.6B", engine="static")
    with pytest.raises(NotImplementedError, match="llama"):
        Qwen3("Qwen/Qwen2.5-7B-Instruct")
    with pytest.raises(NotImplementedError, match="gemma2"):
        Qwen3("google/gemma-2-2b")


def test_qwen3_symbols_templates_alias():
    from umbrella_amd import _lib
    from umbrella_amd.templates import Prompts, SysPrompts
    for n in ("umb_reduce_qkv_rope_qknorm", "umb_model_forward_qwen3", "umb_model_forward_qwen3_offload"):
        assert n in _lib.SIGNATURES
    assert Prompts["qwen3"] == Prompts["qwen"] and SysPrompts["qwen3"] == SysPrompts["qwen"]
    import umbrella.models.qwen3 as m
    from umbrella_amd.models.qwen3 import Qwen3
    assert m.Qwen3 is Qwen3


@pytest.mark.parametrize("kind", sorted(qr.CFGS))
def test_qwen3_ref_reproduces_hf_fixture(kind):
    assert G[kind + "_ref_vs_hf_max_abs"] < 1e-4
    logits = qr.Qwen3Ref(kind).forward(G["prompt"])
    np.testing.assert_allclose(logits.numpy(), LOG[kind + "_logits"], rtol=1e-4, atol=1e-4)
    assert len(G[kind + "_greedy"]) == 48
    assert qr.CFGS[kind]["head_dim"] == 128 and qr.CFGS["A"]["num_attention_heads"] * 128 != qr.CFGS["A"]["hidden_size"]


@pytest.mark.parametrize("kind", sorted(qr.CFGS))
def test_qwen3_fixture_cannot_be_met_without_the_head_norms(kind):
    """The function a runtime computes when it skips q_norm / k_norm (what a Qwen3 directory silently got before this family
    existed) lies at least ten times the GPU logits tolerance away from HF, and its greedy tokens leave HF's before the first
    near-tie at which the engine test stops comparing: neither GPU test can pass on such a runtime"""
    ref = LOG[kind + "_logits"]
    widest = max(tol for tol, _ in LOGIT_TOL.values()) * _tol_scale(ref) + float(np.abs(ref).max()) * 2.0 ** -6
    assert G[kind + "_nonorm_max_abs"] >= 10 * widest, (G[kind + "_nonorm_max_abs"], widest)
    first_tie = next((i for i, x in enumerate(G[kind + "_margins"]) if x < 0.1), len(G[kind + "_margins"]))
    assert G[kind + "_nonorm_first_diff"] < first_tie, (G[kind + "_nonorm_first_diff"], first_tie)
    # and the recorded figures are what the restatement gives today
    off = qr.Qwen3Ref(kind, qk_norm=False).forward(G["prompt"]).numpy()
    assert abs(float(np.abs(off - ref).max()) - G[kind + "_nonorm_max_abs"]) < 1e-3


def test_qwen3_reduce_kernel_neither_spills_nor_uses_scratch_or_lds(tmp_path):
    """a lane keeps its (at most two) pairs of the head in registers from the split sum to the stores: no instantiation of
    reduce_qkv_rope_qknorm_kernel may spill, touch scratch or allocate LDS (per-lane arrays indexed at run time would)"""
    src = os.path.join(ROOT, "umbrella_amd", "csrc", "epilogue.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-mllvm",
                        "-amdgpu-kernarg-preload-count=16", "-c", src, "-o", str(tmp_path / "epilogue.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen = None, {"scratch": 0, "spill": 0, "lds": 0}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        if not (name and "reduce_qkv_rope_qknorm_kernel" in name):
            continue
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m:
                seen[key] += 1
                assert int(m.group(1)) == 0, (name, key, int(m.group(1)))
    assert seen == {"scratch": 4, "spill": 4, "lds": 4}, seen          # 2 dtypes x NP in {1, 2}


# ----------------------------------------------------------------------------- GPU helpers
def _tiny(kind, dtype, max_length=256, sd=None, **kw):
    from umbrella_amd.models.qwen3 import Qwen3
    cfg_kw = {k: kw.pop(k) for k in ("awq",) if k in kw}
    alloc_kw = {k: kw.pop(k) for k in ("num_cache_layers",) if k in kw}
    m = Qwen3("tiny-qwen3-" + kind, max_length=max_length, device="cuda:0", dtype=dtype,
              state_dict=sd if sd is not None else qr.qwen3_state(kind), config=qr.llama_cfg(kind, **cfg_kw), **kw)
    m.alloc(**alloc_kw)
    return m


def _prompt_logits(m, ids):
    n = len(ids)
    mask = torch.tril(torch.ones(n, m.max_length, dtype=torch.bool))
    return m.inference(torch.tensor([ids]), torch.arange(n)[None], mask, torch.arange(n))[0].cpu()


def _ulps_ok(got, want, dtype):
    """the project's criterion for a norm whose 1/rms comes from another summation order (test_gemma2.py): at most one unit of
    the dtype, on fewer than 1 % of the elements"""
    d = (got.float() - want.float()).abs()
    ulp = want.float().abs().clamp_min(1e-30) * (2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10)
    frac = float((d > 0).float().mean())
    print(f"    max diff / ulp {float((d / ulp).max()):.3f}, differing {frac:.5f}")
    return bool((d <= ulp).all()) and frac < 0.01


def _awq_dequant(qweight, qzeros, scales, group=128):
    """AutoAWQ GEMM tensors -> W [N, K] fp32 on their device"""
    from umbrella_amd.models.awq_format import ORDER

    def unpack(p):
        out = torch.empty(p.shape[0], p.shape[1], 8, dtype=torch.int32, device=p.device)
        for i, col in enumerate(ORDER):
            out[:, :, col] = (p >> (4 * i)) & 0xF
        return out.reshape(p.shape[0], p.shape[1] * 8)
    q, z = unpack(qweight).float(), unpack(qzeros).float().repeat_interleave(group, dim=0)
    return ((q - z) * scales.float().repeat_interleave(group, dim=0)).t().contiguous()


# ----------------------------------------------------------------------------- GPU: the kernel
def _run_reduce(name, part, S, T, Hq, Hkv, D, Lmax, pos, slot, cos, sin, paired, bias, ssq, groups, stride, dim, eps, qw, kw,
                dtype):
    from umbrella_amd import _lib
    dev = part.device
    q = torch.zeros(T, Hq, D, dtype=dtype, device=dev)
    kc = torch.zeros(Hkv * Lmax * D, dtype=dtype, device=dev)
    vt = torch.zeros(Hkv * D * (Lmax + 32), dtype=dtype, device=dev)
    args = [part, S, T, Hq, Hkv, D, Lmax, pos, slot, cos, sin, q, kc, vt, paired, bias, ssq, groups, stride, dim, eps]
    if name == "umb_reduce_qkv_rope_qknorm":
        args += [qw, kw, 1e-6]
    _lib.call(name, *args, _lib.dtype_code(dtype))
    torch.cuda.synchronize()
    return q, kc, vt


def _cache_rows(kc, vt, slots, Hkv, D, Lmax):
    """K / V [T, Hkv, D] of the keys `slots`, read through the layout's Python mirror"""
    from umbrella_amd.attn.cache import k_offsets, vt_offsets
    k = kc.view(Hkv, Lmax * D)[:, k_offsets(slots.long(), D)]                      # [Hkv, T, D]
    v = vt.view(Hkv, D * (Lmax + 32))[:, vt_offsets(slots.long(), D).t()]
    return k.permute(1, 0, 2).contiguous(), v.permute(1, 0, 2).contiguous()


def _appended(k, v, slots, Hkv, D, Lmax, dtype):
    """the caches umb_kv_append builds from K / V [T, Hkv, D] at `slots` (every other element zero)"""
    from umbrella_amd import _lib
    dev = k.device
    kc = torch.zeros(Hkv * Lmax * D, dtype=dtype, device=dev)
    vt = torch.zeros(Hkv * D * (Lmax + 32), dtype=dtype, device=dev)
    _lib.call("umb_kv_append", kc, vt, k.to(dtype).contiguous(), v.to(dtype).contiguous(), slots, k.shape[0], Hkv, D, Lmax,
              _lib.dtype_code(dtype))
    return kc, vt


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("S", [1, 3, 9])
def test_qwen3_reduce_qknorm_rope_op(dtype, D, S):
    """umb_reduce_qkv_rope_qknorm: rows at position 0 (RoPE is the identity) against the restatement within one unit of the
    dtype; the same partials at scattered positions / slots equal, bit for bit, the restatement's RoPE of the kernel's own
    position-0 output, K and V^T in umb_kv_append's layout; V equals the plain kernel's bit for bit.

    One unit of a head norm's input can become two of round(w * round(x * r)), so the criterion can only hold where the two
    sides agree on both 1/rms factors: the restatement adds the squares in the kernel's documented order (qr.head_sumsq, the
    64-lane butterfly) and both form 1 / sqrt correctly rounded.  v rows keep reduce_qkv_rope_kernel's estimate of the token's
    1/rms and differ from the restatement by at most one unit, rarely."""
    dev = torch.device("cuda:0")
    T, Hq, Hkv, Lmax, H = 7, 4, 2, 96, 1024
    N = (Hq + 2 * Hkv) * D
    g = torch.Generator(device=dev).manual_seed(100 * D + S)
    cos, sin = (t.to(dev).contiguous() for t in qr.rope_tables(D, 1e6, Lmax, dtype))
    cos, sin = cos.to(dtype), sin.to(dtype)
    qw = (2.0 + 0.4 * torch.randn(D, device=dev, generator=g)).to(dtype)      # the op test keeps weights of magnitude 2 / 1.5
    kw = (1.5 + 0.4 * torch.randn(D, device=dev, generator=g)).to(dtype)
    pos0 = torch.zeros(T, dtype=torch.int32, device=dev)
    slot0 = torch.arange(T, dtype=torch.int32, device=dev)
    posp = torch.tensor([3, 0, 8, 20, 95, 41, 64], dtype=torch.int32, device=dev)
    slotp = torch.tensor([0, 5, 2, 33, 95, 63, 64], dtype=torch.int32, device=dev)
    half = D // 2
    for use_ssq in (False, True):
        for use_bias in (False, True):
            hf = torch.randn(S, T, N, device=dev, generator=g) * (3.0 if use_ssq else 1.0)      # HF feature order
            bias = (torch.randn(N, device=dev, generator=g) * 0.5).to(dtype) if use_bias else None
            groups, stride = H // 64, 32
            ssq = (torch.rand(T, stride, device=dev, generator=g) * 64 * 9.0) if use_ssq else None
            acc = hf[0]
            for s in range(1, S):
                acc = acc + hf[s]
            if use_ssq:
                # the token's sums of squares as the kernel adds them: one per lane, then the butterfly
                tot = qr.butterfly_sum(torch.nn.functional.pad(ssq[:, :groups], (0, 64 - groups)))
                acc = acc * (1.0 / torch.sqrt((tot[:, None] / H + 1e-5).double())).float()      # 1 / rms correctly rounded
            want_q, want_k, want_v = qr.qk_norm_rope(acc, Hq, Hkv, D, qw, kw, 1e-6, cos[pos0.long()], sin[pos0.long()], dtype, bias)
            for paired in (0, 1):
                part = hf
                if paired:                                   # repack mode 2: columns (2d, 2d + 1) <-> features (d, d + D/2)
                    v4 = hf.view(S, T, Hq + 2 * Hkv, D)
                    pp = v4.clone()
                    pp[:, :, :Hq + Hkv, 0::2] = v4[:, :, :Hq + Hkv, :half]
                    pp[:, :, :Hq + Hkv, 1::2] = v4[:, :, :Hq + Hkv, half:]
                    part = pp.view(S, T, N).contiguous()
                tail = (paired, bias, ssq, groups if use_ssq else 0, stride if use_ssq else 0, float(H) if use_ssq else 0.0,
                        1e-5 if use_ssq else 0.0, qw, kw, dtype)
                print(f"  D {D} S {S} ssq {use_ssq} bias {use_bias} paired {paired}")
                q0, kc0, vt0 = _run_reduce("umb_reduce_qkv_rope_qknorm", part, S, T, Hq, Hkv, D, Lmax, pos0, slot0, cos, sin, *tail)
                k0, v0 = _cache_rows(kc0, vt0, slot0, Hkv, D, Lmax)
                kc_chk, vt_chk = _appended(k0, v0, slot0, Hkv, D, Lmax, dtype)
                assert torch.equal(kc0, kc_chk) and torch.equal(vt0, vt_chk)           # nothing outside the rows' slots
                assert _ulps_ok(q0, want_q, dtype) and _ulps_ok(k0, want_k, dtype) and _ulps_ok(v0, want_v, dtype)
                # scattered positions and slots: RoPE of the kernel's own position-0 rows, bit for bit
                qp, kcp, vtp = _run_reduce("umb_reduce_qkv_rope_qknorm", part, S, T, Hq, Hkv, D, Lmax, posp, slotp, cos, sin, *tail)
                cp, sp = cos[posp.long()], sin[posp.long()]
                assert torch.equal(qp.float(), qr.rope_rounded(q0.float(), cp, sp, dtype))
                kc_want, vt_want = _appended(qr.rope_rounded(k0.float(), cp, sp, dtype), v0, slotp, Hkv, D, Lmax, dtype)
                assert torch.equal(kcp, kc_want) and torch.equal(vtp, vt_want)
                # V against the kernel without the head norm
                _, _, vt_plain = _run_reduce("umb_reduce_qkv_rope2", part, S, T, Hq, Hkv, D, Lmax, posp, slotp, cos, sin, *tail)
                assert torch.equal(vtp, vt_plain)


# ----------------------------------------------------------------------------- GPU: model
@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(qr.CFGS))
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_qwen3_logits_vs_fixture(kind, dtype):
    """HIP runtime vs HF's fp32 logits (tolerances and formula of test_gemma2_logits_vs_fixture); offloaded == resident bit
    for bit."""
    tol, rel = LOGIT_TOL[dtype]
    outs = []
    for offload in (False, True):
        m = _tiny(kind, dtype, offload=offload)
        logits = _prompt_logits(m, G["prompt"])
        ref = torch.from_numpy(LOG[kind + "_logits"])
        scale = _tol_scale(ref)
        err = (logits - ref).abs()
        print(f"  {kind} {dtype} offload {offload}: max err {float(err.max()):.4f} (bound {tol * scale:.4f} + rel)")
        assert (err <= tol * scale + ref.abs() * rel).all(), float(err.max())
        assert (logits.argmax(-1) == ref.argmax(-1)).float().mean() > 0.9
        outs.append(logits)
        del m
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(qr.CFGS))
def test_qwen3_awq_logits_vs_dequantised_fp32(kind):
    """the tiny model quantised to AutoAWQ tensors: the runtime against the fp32 forward of the DEQUANTISED weights"""
    from umbrella_amd.models.synthetic import awq_quantize_small
    dtype = torch.float16
    sd = qr.qwen3_state(kind)
    awq, deq = {}, {}
    for k, v in sd.items():
        if k.endswith("_proj.weight"):
            qw, qz, sc = awq_quantize_small(v, 128)
            base = k[:-len(".weight")]
            awq[base + ".qweight"], awq[base + ".qzeros"], awq[base + ".scales"] = qw, qz, sc
            deq[k] = _awq_dequant(qw, qz, sc)
        else:
            awq[k] = deq[k] = v
    m = _tiny(kind, dtype, sd=awq, awq=True)
    assert m.layers[0]["qkv"].awq
    logits = _prompt_logits(m, G["prompt"])
    ref = qr.Qwen3Ref(kind, deq).forward(G["prompt"])
    tol, rel = LOGIT_TOL[dtype]
    err = (logits - ref).abs()
    print(f"  {kind} awq: max err {float(err.max()):.4f}")
    assert (err <= tol * _tol_scale(ref) + ref.abs() * rel).all(), float(err.max())


@pytest.mark.gpu
def test_qwen3_graph_equals_eager():
    m = _tiny("A", torch.bfloat16, cuda_graph=True)
    dev = torch.device("cuda:0")
    T = len(G["prompt"])
    ids = torch.tensor(G["prompt"], dtype=torch.int32, device=dev)
    pos = torch.arange(T, dtype=torch.int32, device=dev)
    pre = torch.zeros(1, dtype=torch.int32, device=dev)
    m.forward_explicit(ids, pos, pos, pre, head_from=0)
    eager = m.logits_buffer[:T].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.forward_explicit(ids, pos, pos, pre, head_from=0)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.forward_explicit(ids, pos, pos, pre, head_from=0)
    m.logits_buffer.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(m.logits_buffer[:T], eager)


@pytest.mark.gpu
def test_qwen3_out_of_scope_raises():
    from umbrella_amd.models.qwen3 import Qwen3
    m = Qwen3("x", device="cuda:0", state_dict=qr.qwen3_state("A"), config=qr.llama_cfg("A"))
    with pytest.raises(NotImplementedError):
        m.alloc(layer_range=(0, 2))
    m = _tiny("A", torch.float16)
    m.use_gemv(True)                                  # no-op
    assert not m.gemv and not getattr(m, "chain", False) and not m._ws.chain_xchg and m._ws.fused == 0
    assert all(not getattr(ln, "gemv_on", False) and getattr(ln, "w_rows", None) is None for ln in m.layers[0].values())
    m._tp = object()
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        _prompt_logits(m, G["prompt"][:4])


def _width_state(cfg, dev, dtype, awq, seed=5):
    """two layers of seeded weights at a published width, scaled as tests/qwen3_ref.qwen3_state; returns (runtime state dict,
    fp32 dense state dict of the same function)"""
    from umbrella_amd.models.synthetic import linear_shapes, synth_awq_tensors
    g = torch.Generator(device=dev).manual_seed(seed)
    H, V, D = cfg.hidden_size, cfg.vocab_size, cfg.head_dim

    def rn(*shape, s):
        return (torch.randn(*shape, device=dev, generator=g) * s).to(dtype)
    # logits of std 3, as in test_gemma2_full_width_two_layers whose bounds this test takes (final norm 3 on a head of std
    # H^-1/2 there): a tied head is the embedding (std 0.25), so the final norm's mean carries the scale
    tied = cfg.tie_word_embeddings
    sd = {"model.embed_tokens.weight": rn(V, H, s=0.25),
          "model.norm.weight": rn(H, s=0.1) * (12.0 * H ** -0.5 if tied else 2.0) + (12.0 * H ** -0.5 if tied else 2.0)}
    if not tied:
        sd["lm_head.weight"] = rn(V, H, s=1.5 * H ** -0.5)
    ref = {k: v.float() for k, v in sd.items()}
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        for n, (a, b) in linear_shapes(cfg).items():
            s = (3.0 if n.endswith("o_proj") else 1.0) * b ** -0.5
            if awq:
                qw, qz, sc = synth_awq_tensors(a, b, 128, dev, g, s)
                sd[p + n + ".qweight"], sd[p + n + ".qzeros"], sd[p + n + ".scales"] = qw, qz, sc
                ref[p + n + ".weight"] = _awq_dequant(qw, qz, sc)
            else:
                sd[p + n + ".weight"] = rn(a, b, s=s)
                ref[p + n + ".weight"] = sd[p + n + ".weight"].float()
        for n, (mean, std), shape in (("input_layernorm", (1.0, 0.2), H), ("post_attention_layernorm", (1.0, 0.2), H),
                                      ("self_attn.q_norm", qr.Q_NORM, D), ("self_attn.k_norm", qr.K_NORM, D)):
            sd[p + n + ".weight"] = rn(shape, s=std) + mean
            ref[p + n + ".weight"] = sd[p + n + ".weight"].float()
    return sd, ref


_WIDTH_CHILD = """
import sys, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_qwen3 as t
torch.save(t._width_logits({name!r}, {T}), {out!r})
"""


def _width_logits(name, T):
    """(runtime logits [T, V], fp32 restatement, restatement without the head norms) of two layers at `name`'s width over a
    T-token causal prompt in one forward"""
    from umbrella_amd.models.config import KNOWN
    from umbrella_amd.models.qwen3 import Qwen3
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    cfg = dataclasses.replace(KNOWN[name], num_hidden_layers=2)
    sd, ref_sd = _width_state(cfg, dev, dtype, cfg.awq)
    m = Qwen3(name, max_length=256, device=str(dev), dtype=dtype, state_dict=sd, config=cfg)
    m.alloc()
    ids = torch.randint(0, cfg.vocab_size, (T,), generator=torch.Generator().manual_seed(1)).tolist()
    got = _prompt_logits(m, ids)
    c = dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
             num_hidden_layers=2, num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads,
             head_dim=cfg.head_dim, tie_word_embeddings=cfg.tie_word_embeddings, **qr.COMMON)
    ref = qr.Qwen3Ref(c, ref_sd).forward(ids).cpu()
    off = qr.Qwen3Ref(c, ref_sd, qk_norm=False).forward(ids).cpu()
    defer = bool(m._ws.defer_norm) and cfg.hidden_size % 2048 == 0
    del m
    torch.cuda.empty_cache()
    return got, ref, off, defer


@pytest.mark.gpu
@pytest.mark.parametrize("name,T", [("Qwen/Qwen3-1.7B", 13), ("Qwen/Qwen3-1.7B", 32), ("Qwen/Qwen3-32B-AWQ", 13),
                                    ("Qwen/Qwen3-32B-AWQ", 32), ("Qwen/Qwen3-0.6B", 13), ("Qwen/Qwen3-0.6B", 32)])
def test_qwen3_full_width_two_layers(name, T, tmp_path):
    """two layers at the published dims vs the fp32 restatement on the GPU, 13 rows (row-major) and 32 rows (FM order), bounds
    of test_gemma2_full_width_two_layers: 1.7B (H 2048) takes the deferred-norm layer, 32B-AWQ and 0.6B the in-place one.
    1.7B also with UMB_DEFER_NORM=0 in a child process: the same function through the other reduce, so it meets the same
    bounds and lies within the two runs' summed 16-bit error of the deferred result"""
    got, ref, off, defer = _width_logits(name, T)
    assert defer == (name == "Qwen/Qwen3-1.7B")
    err, wrong = float((got - ref).abs().max()), float((off - ref).abs().max())
    print(f"  {name} T {T}: err {err:.4f}, without the head norms {wrong:.4f}, max |logit| {float(ref.abs().max()):.2f}")
    assert err < 0.3 * wrong, (err, wrong)
    assert err < 0.5, err
    if not defer:
        return
    out = str(tmp_path / "nodefer.pt")
    code = _WIDTH_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), name=name, T=T, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, UMB_DEFER_NORM="0"), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got2, ref2, _, defer2 = torch.load(out)
    assert not defer2 and torch.equal(ref2, ref)
    err2, diff = float((got2 - ref).abs().max()), float((got2 - got).abs().max())
    print(f"  UMB_DEFER_NORM=0: err {err2:.4f}, to the deferred run {diff:.4f}")
    assert err2 < 0.3 * wrong and err2 < 0.5, err2
    assert diff <= err + err2 + 1e-6 and diff < 0.5, diff


def _engine(kind_t, draft, engine, **kw):
    from umbrella_amd.speculation.dynamic_speculation_engine import DynamicSpeculationEngine
    from umbrella_amd.speculation.speculation_utils import IdTokenizer
    from umbrella_amd.speculation.static_speculation_engine import StaticSpeculationEngine
    dtype = torch.float16
    target = _tiny(kind_t, dtype)
    if draft == "llama":
        from hip_helpers import hip_model
        cfgd = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                    num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-5, rope_theta=10000.0, max_position_embeddings=2048,
                    tie_word_embeddings=True)
        draft, _ = hip_model(cfgd, 7, 256, dtype, "cuda:0", cuda_graph=(engine == "static"))
    else:
        draft = _tiny(draft, dtype, cuda_graph=(engine == "static"))
    common = dict(dtype=dtype, device="cuda:0", max_length=256, safe_buffer=16, stop_distance=8, draft_model_obj=draft,
                  target_model_obj=target, tokenizer=IdTokenizer())
    if engine == "static":
        return StaticSpeculationEngine("d", "t", growmap=GM["3x4"], **common)
    return DynamicSpeculationEngine("d", "t", width=kw.get("width", 4), num_beams=kw.get("num_beams", 8),
                                    depth=kw.get("depth", 6), **common)


@pytest.mark.gpu
@pytest.mark.parametrize("engine,draft", [("static", "B"), ("dynamic", "B"), ("static", "llama")])
def test_qwen3_engines_follow_greedy_target(engine, draft):
    """Qwen3 target (A) with a Qwen3 draft (B) in both engines, and with a Llama-family draft on its own schedule: every
    emitted token is an arg-max of the fp32 target within the 16-bit slack, and HF's greedy token up to the first recorded
    near-tie"""
    eng = _engine("A", draft, engine)
    eng.initialize()
    if draft == "llama":
        assert type(eng.draft_model).__name__ == "Llama" and eng.draft_model._ws.fused == 2
    assert eng.target_model._ws.fused == 0 and not eng.target_model.gemv
    prompt = G["prompt"]
    out = eng.generate(input_ids=prompt, max_new_tokens=48)
    toks = out["generated_tokens"]
    assert len(toks) >= 1
    seq = list(prompt) + toks
    logits = qr.Qwen3Ref("A").forward(seq)
    for i, tok in enumerate(toks):
        row = logits[len(prompt) + i - 1].clone()
        if i == 0 and engine == "dynamic":
            row[[3, 5]] = -float("inf")
        assert float(row.max() - row[tok]) <= 0.1, (i, tok, float(row.max() - row[tok]))
    hf, margins = G["A_greedy"], G["A_margins"]
    for i in range(min(len(toks), len(hf))):
        if margins[i] < 0.1:
            break
        assert toks[i] == hf[i], (i, toks[:i + 1], hf[:i + 1])


@pytest.mark.gpu
def test_qwen3_32b_awq_target_06b_draft_full_depth(monkeypatch):
    """AutoModelLM.from_pretrained("Qwen/Qwen3-32B-AWQ") end to end with the 0.6B as draft, synthetic weights, static 3x4:
    every emitted token is an arg-max of the 32B's own eager logits over the sequence (within the 16-bit tie margin of
    test_gemma2_27b_target_2b_draft_full_depth).  Row counts stay at the 24-token prompt chunk and the 13-row tree: outside
    the prefill widths of DESIGN.md's empty-split list"""
    from umbrella_amd.models.auto_model import AutoModelLM
    from umbrella_amd.models.qwen3 import Qwen3
    from umbrella_amd.speculation.speculation_utils import IdTokenizer
    from umbrella_amd.speculation.static_speculation_engine import StaticSpeculationEngine
    monkeypatch.setenv("UMBRELLA_SYNTHETIC", "1")
    dtype = torch.float16
    target = AutoModelLM.from_pretrained("Qwen/Qwen3-32B-AWQ", dtype=dtype, max_length=256)
    draft = AutoModelLM.from_pretrained("Qwen/Qwen3-0.6B", dtype=dtype, max_length=256, cuda_graph=True)
    assert isinstance(target, Qwen3) and isinstance(draft, Qwen3)
    target.alloc()
    draft.alloc()
    eng = StaticSpeculationEngine("Qwen/Qwen3-0.6B", "Qwen/Qwen3-32B-AWQ", growmap=GM["3x4"], dtype=dtype,
                                  device="cuda:0", max_length=256, safe_buffer=16, stop_distance=8, draft_model_obj=draft,
                                  target_model_obj=target, tokenizer=IdTokenizer())
    eng.initialize()
    prompt = torch.randint(1000, 150000, (24,), generator=torch.Generator().manual_seed(2)).tolist()
    out = eng.generate(input_ids=prompt, max_new_tokens=40)
    toks = out["generated_tokens"]
    assert len(toks) >= 8
    seq = prompt + toks
    target.clear()
    n = len(seq)
    logits = target.inference(torch.tensor([seq]), torch.arange(n)[None], torch.tril(torch.ones(n, 256, dtype=torch.bool)),
                              torch.arange(n))[0]
    for i, tok in enumerate(toks):
        row = logits[len(prompt) + i - 1]
        assert float(row.max() - row[tok]) <= 0.25, (i, tok, float(row.max() - row[tok]))
    del eng, target, draft
    torch.cuda.empty_cache()
