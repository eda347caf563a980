"""Gemma-2 (2B / 9B / 27B) on the HIP path: config and registry, the CPU restatement against HF's recorded logits, and on
the GPU the new kernels (soft-capped / windowed D = 128 / 256 attention, Gemma norms, the sandwich reduce, GELU * up, the
final soft-cap), the whole model against the fixture and both engines with a Gemma target and draft.

Fixture: tests/golden/make_golden_gemma2.py (HF Gemma2ForCausalLM, fp32, eager).  GPU tests read the fixture and
tests/gemma2_ref.py only."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import gemma2_ref as gr
from helpers import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(GOLD, "gemma2.json")) as f:
    G = json.load(f)
LOG = np.load(os.path.join(GOLD, "gemma2_logits.npz"))
with open(os.path.join(GOLD, "growmaps.json")) as f:
    GM = json.load(f)
DTYPES = [torch.float16, torch.bfloat16]


# ----------------------------------------------------------------------------- CPU
def test_gemma2_registry_traits():
    from umbrella_amd.models.auto_model import AutoModelLM
    from umbrella_amd.models.config import KNOWN
    from umbrella_amd.models.gemma import Gemma2
    ids = ("google/gemma-2-2b", "google/gemma-2-2b-it", "google/gemma-2-9b-it", "google/gemma-2-27b-it")
    for name in ids:
        c = KNOWN[name]
        assert c.family == "gemma2" and c.vocab_size == 256000 and c.tie_word_embeddings
        assert (c.attn_logit_softcapping, c.final_logit_softcapping, c.sliding_window) == (50.0, 30.0, 4096)
        assert c.hidden_activation == "gelu_pytorch_tanh" and c.is_sliding(0) and not c.is_sliding(1)
        for table in (AutoModelLM._MODEL_MAPPING, AutoModelLM._OFFLOAD_MODEL_MAPPING, AutoModelLM._CUDAGRAPH_MODEL_MAPPING):
            assert table[name] is Gemma2
    assert KNOWN["google/gemma-2-2b"].head_dim == 256 and KNOWN["google/gemma-2-9b-it"].head_dim == 256
    assert KNOWN["google/gemma-2-27b-it"].head_dim == 128
    assert abs(KNOWN["google/gemma-2-27b-it"].attn_scale - 1.0 / 12.0) < 1e-12
    assert abs(KNOWN["google/gemma-2-9b-it"].attn_scale - 1.0 / 16.0) < 1e-12
    assert KNOWN["google/gemma-2-27b-it"].eos_token_id == [1, 107]
    # every other family keeps its defaults
    ll = KNOWN["meta-llama/Llama-3.1-8B-Instruct"]
    assert ll.family == "llama" and ll.sliding_window == 0 and ll.attn_scale == 128 ** -0.5


def test_gemma2_from_dir(tmp_path):
    from umbrella_amd.models.auto_model import _dir_class
    from umbrella_amd.models.config import LlamaCfg
    from umbrella_amd.models.gemma import Gemma2
    cfg = {"model_type": "gemma2", "vocab_size": 512, "hidden_size": 256, "intermediate_size": 512, "num_hidden_layers": 4,
           "num_attention_heads": 4, "num_key_value_heads": 2, "head_dim": 128, "rms_norm_eps": 1e-6,
           "rope_parameters": {"rope_type": "default", "rope_theta": 10000.0}, "query_pre_attn_scalar": 144,
           "sliding_window": 16, "attn_logit_softcapping": 50.0, "final_logit_softcapping": 30.0,
           "hidden_activation": "gelu_pytorch_tanh", "tie_word_embeddings": True, "eos_token_id": 1,
           "layer_types": ["sliding_attention", "full_attention"] * 2}
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    (tmp_path / "generation_config.json").write_text(json.dumps({"eos_token_id": [1, 107]}))
    c = LlamaCfg.from_dir(str(tmp_path))
    assert c.family == "gemma2" and c.head_dim == 128 and abs(c.attn_scale - 1 / 12) < 1e-12
    assert (c.sliding_window, c.sliding_parity, c.eos_token_id) == (16, 0, [1, 107])
    assert c.rope_theta == 10000.0 and c.tie_word_embeddings and not c.awq
    assert _dir_class(str(tmp_path)) is Gemma2
    cfg["layer_types"] = ["full_attention", "full_attention", "sliding_attention", "full_attention"]
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    with pytest.raises(NotImplementedError):
        LlamaCfg.from_dir(str(tmp_path))
    # keys missing from config.json take HF Gemma2Config's defaults, an explicit null turns the feature off
    for k in ("query_pre_attn_scalar", "sliding_window", "attn_logit_softcapping", "final_logit_softcapping", "layer_types"):
        cfg.pop(k)
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    c = LlamaCfg.from_dir(str(tmp_path))
    assert (c.query_pre_attn_scalar, c.sliding_window, c.attn_logit_softcapping, c.final_logit_softcapping) == (256, 4096, 50, 30)
    cfg["final_logit_softcapping"] = None
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    assert LlamaCfg.from_dir(str(tmp_path)).final_logit_softcapping == 0.0


def test_gemma2_config_never_reaches_the_llama_runtime():
    """plain Llama, the tensor-parallel and the layer-pipelined builders would run SiLU / Llama norms / 1/sqrt(D) on a
    Gemma-2 config: each refuses it before touching a device or a process group"""
    from umbrella_amd.models.config import KNOWN
    from umbrella_amd.models.gemma import Gemma2
    from umbrella_amd.models.llama import Llama
    from umbrella_amd.parallel import build_pipelined_engine
    from umbrella_amd.tensor_parallel import TensorParallelLlama, build_tp_engine
    name = "google/gemma-2-27b-it"
    with pytest.raises(NotImplementedError, match="gemma2"):
        Llama(name)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        TensorParallelLlama.build(KNOWN[name], {}, None, 256, "cpu", torch.bfloat16)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        build_tp_engine("cpu", model=name, draft_model="google/gemma-2-2b-it", engine="static")
    with pytest.raises(NotImplementedError, match="layer pipelining"):
        build_pipelined_engine("cpu", model=name, draft_model="google/gemma-2-2b-it", engine="static")
    with pytest.raises(NotImplementedError, match="llama"):
        Gemma2("meta-llama/Llama-3.2-1B-Instruct")


@pytest.mark.parametrize("kind", sorted(gr.CFGS))
def test_gemma2_ref_reproduces_hf_fixture(kind):
    assert G[kind + "_ref_vs_hf_max_abs"] < 1e-4
    logits = gr.Gemma2Ref(kind).forward(G["prompt"])
    np.testing.assert_allclose(logits.numpy(), LOG[kind + "_logits"], rtol=1e-4, atol=1e-4)
    assert len(G[kind + "_greedy"]) == 48 and min(G[kind + "_margins"]) > 0.05


def test_gemma_module_resolves_through_alias():
    import umbrella.models.gemma as m
    from umbrella_amd.models.gemma import Gemma2
    assert m.Gemma2 is Gemma2


def test_gemma2_attention_kernels_neither_spill_nor_use_scratch(tmp_path):
    """D = 256 holds O^T (64 VGPRs) + one K and V^T tile (128) in registers: no instantiation of the Gemma path may spill."""
    src = os.path.join(ROOT, "umbrella_amd", "csrc", "attn.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-mllvm",
                        "-amdgpu-kernarg-preload-count=16", "-c", src, "-o", str(tmp_path / "attn.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen = None, 0
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        if not (name and "tree_attn1_kernel" in name and name.endswith("Lb1EEvPKtS2_S2_PKiiiiiiiPKyfPtiPfS8_PjiiS4_fi")):
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            seen += 1
            assert int(m.group(1)) == 0, (name, "scratch", int(m.group(1)))
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m:
            assert int(m.group(1)) == 0, (name, "spilled VGPRs", int(m.group(1)))
    assert seen == 2 * 2 * 3                  # 2 dtypes x D in {128, 256} x 3 wave counts


# ----------------------------------------------------------------------------- GPU helpers
def _attn_case(dtype, D, Hq, Hkv, T, start, window, cap, tree, Lmax=2048, seed=0):  # noqa: C901
    """Run umb_tree_attn_gemma2 on one case; returns (kernel out, fp32 reference), both [T, Hq, D] fp32 on the CPU.
    tree: rows are a random tree of T nodes behind a `start`-key prefix (positions start + depth); else causal prefill.
    K / V slots below the 32-key tile holding the first key any row can see are NaN: reading one poisons the output."""
    from umbrella_amd import _lib
    from umbrella_amd.models.llama import pack_mask_bits
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    C = start + T
    scale = 1.0 / 12.0 if D == 128 else 1.0 / 16.0
    qs = 6.0 if cap else 1.0                               # large scores when the cap is on: tanh leaves its linear range
    q = (torch.randn(T, Hq, D, generator=g) * qs).to(dtype)
    k = torch.randn(C, Hkv, D, generator=g).to(dtype)
    v = torch.randn(C, Hkv, D, generator=g).to(dtype)
    if tree:
        parent = [-1] + [int(torch.randint(0, i, (1,), generator=g)) for i in range(1, T)]
        depth = [0] * T
        anc = torch.zeros(T, T, dtype=torch.bool)
        for i in range(T):
            anc[i, i] = True
            if parent[i] >= 0:
                depth[i] = depth[parent[i]] + 1
                anc[i] |= anc[parent[i]]
        qpos = torch.tensor([start + d for d in depth], dtype=torch.int32)
        bits = pack_mask_bits(anc)
        vis = torch.zeros(T, C, dtype=torch.bool)
        vis[:, :start] = True
        vis[:, start:] = anc
        assert not window or max(depth) < window
    else:
        qpos = torch.arange(start, start + T, dtype=torch.int32)
        bits = None
        vis = torch.arange(C)[None] <= qpos[:, None].long()
    if window:
        vis &= (qpos[:, None].long() - torch.arange(C)[None]) < window
    ref = gr.attention(q.float(), k.float(), v.float(), scale, cap, vis)
    kg, vg = k.clone(), v.clone()
    poison = 0
    if window:
        poison = max(int(qpos.min()) - window + 1, 0) // 32 * 32
        kg[:poison] = float("nan")
        vg[:poison] = float("nan")
    kc = torch.zeros(Hkv * Lmax * D, dtype=dtype, device=dev)
    vt = torch.zeros(Hkv * D * (Lmax + 32), dtype=dtype, device=dev)
    slots = torch.arange(C, dtype=torch.int32, device=dev)
    _lib.call("umb_kv_append", kc, vt, kg.to(dev).contiguous(), vg.to(dev).contiguous(), slots, C, Hkv, D, Lmax,
              _lib.dtype_code(dtype))
    splits = 16
    po = torch.zeros(splits * T * Hq * D, dtype=torch.float32, device=dev)
    pml = torch.zeros(splits * T * Hq * 2, dtype=torch.float32, device=dev)
    counters = torch.zeros(Hkv * ((T * (Hq // Hkv) + 15) // 16) + 64, dtype=torch.int32, device=dev)
    out = torch.zeros(T, Hq, D, dtype=dtype, device=dev)
    prefix = torch.tensor([start], dtype=torch.int32, device=dev)
    W = bits.shape[1] if bits is not None else 0
    _lib.call("umb_tree_attn_gemma2", out, q.to(dev).contiguous(), kc, vt, po, pml, prefix,
              bits.to(dev).contiguous() if bits is not None else None, W, T, T, Hq, Hkv, D, Lmax, splits, scale, float(cap),
              qpos.to(dev), window, counters, _lib.dtype_code(dtype))
    torch.cuda.synchronize()
    assert int(counters.abs().sum()) == 0                     # self-resetting span counters
    return out.float().cpu(), ref, poison


def _tiny(kind, dtype, max_length=256, **kw):
    from umbrella_amd.models.gemma import Gemma2
    alloc_kw = {k: kw.pop(k) for k in ("num_cache_layers",) if k in kw}
    m = Gemma2("tiny-gemma2-" + kind, max_length=max_length, device="cuda:0", dtype=dtype, state_dict=gr.gemma2_state(kind),
               config=gr.llama_cfg(kind), **kw)
    m.alloc(**alloc_kw)
    return m


def _prompt_logits(m, ids):
    n = len(ids)
    mask = torch.tril(torch.ones(n, m.max_length, dtype=torch.bool))
    return m.inference(torch.tensor([ids]), torch.arange(n)[None], mask, torch.arange(n))[0].cpu()


# ----------------------------------------------------------------------------- GPU: kernels
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("case", [
    # (T, start, window, cap, tree)
    (40, 0, 16, 50.0, False),          # prompt crossing the window, one span
    (40, 0, 0, 50.0, False),           # global layer
    (13, 300, 64, 20.0, True),         # tree behind a prefix, window 64
    (13, 300, 16, 0.0, True),          # cap off, window 16 (tree depth < 16)
    (64, 1500, 64, 20.0, False),       # 512-key spans: the window starts in span 2, spans 2 and 3 live and merged
    (13, 1500, 700, 0.0, True),        # windowed, two live spans merged (span 0 skipped)
    (13, 1500, 0, 20.0, True),         # global, three spans merged
    (256, 0, 64, 20.0, False, 32, 16),  # 512 (kv head, query tile) blocks: two waves per block
    (900, 0, 64, 20.0, False, 32, 16),  # >= 1792 blocks: one wave per block
    (900, 0, 0, 0.0, False, 32, 16),
])
def test_gemma2_attention_vs_ref(dtype, D, case):
    T, start, window, cap, tree = case[:5]
    Hq, Hkv = case[5:] if len(case) > 5 else ((8, 4) if D == 256 else (16, 8))
    out, ref, poison = _attn_case(dtype, D, Hq, Hkv, T, start, window, cap, tree)
    assert torch.isfinite(out).all(), f"NaN: a key slot below {poison} was read"
    tol = 2.5e-2 if dtype == torch.bfloat16 else 4e-3
    err = float((out - ref).abs().max())
    assert err <= tol, err


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemma_norm_sandwich_gelu_softcap(dtype):
    from umbrella_amd import _lib
    dev = torch.device("cuda:0")
    dc = _lib.dtype_code(dtype)
    g = torch.Generator(device=dev).manual_seed(3)
    T, H, I, S, eps = 13, 2304, 512, 3, 1e-6

    def ulps_ok(got, want):                      # the row's 1/rms comes from another summation order: <= 1 ulp, rarely
        d = (got.float() - want.float()).abs()
        ulp = want.float().abs().clamp_min(1e-30) * (2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10)
        return bool((d <= ulp).all()) and float((d > 0).float().mean()) < 0.01
    # Gemma RMSNorm with the embedding scale folded in front
    x = (torch.randn(T, H, device=dev, generator=g) * 3).to(dtype)
    w = (torch.randn(H, device=dev, generator=g) * 0.3).to(dtype)
    sc = float(torch.tensor(H ** 0.5, dtype=dtype))
    x0 = x.clone()
    xn = torch.empty_like(x)
    _lib.call("umb_gemma_rmsnorm", xn, x, w, eps, sc, T, H, dc)
    xs = (x0.float() * sc).to(dtype)
    assert torch.equal(x, xs)                                        # h <- round(h * round(sqrt H)), bit for bit
    assert ulps_ok(xn, gr.gemma_norm(xs, w, eps, dtype))
    # sandwich reduce
    part = torch.randn(S, T, H, device=dev, generator=g) * 2
    h = (torch.randn(T, H, device=dev, generator=g) * 4).to(dtype)
    wp, wn = [(torch.randn(H, device=dev, generator=g) * 0.3).to(dtype) for _ in range(2)]
    hsum = part[0]
    for s in range(1, S):
        hsum = hsum + part[s]
    h_ref, xn_ref = gr.sandwich(hsum, h, wp, wn, eps, dtype)
    h_gpu, xn_gpu = h.clone(), torch.empty_like(h)
    _lib.call("umb_gemma_sandwich", part, S, T, H, h_gpu, xn_gpu, wp, wn, eps, dc)
    assert ulps_ok(h_gpu, h_ref) and ulps_ok(xn_gpu, xn_ref)
    h_only = h.clone()
    _lib.call("umb_gemma_sandwich", part, S, T, H, h_only, None, wp, None, eps, dc)
    assert torch.equal(h_only, h_gpu)
    # GELU-tanh * up on [gate | up] partials
    pg = torch.randn(S, T, 2 * I, device=dev, generator=g)
    act = torch.empty(T, I, dtype=dtype, device=dev)
    _lib.call("umb_reduce_gelu_mul", pg, S, T, I, act, dc)
    tot = pg[0]
    for s in range(1, S):
        tot = tot + pg[s]
    want = gr.gelu_mul(tot[:, :I], tot[:, I:], dtype)
    assert ulps_ok(act, want)
    # final soft-cap
    z = torch.randn(5, 1000, device=dev, generator=g) * 80
    zc = z.clone()
    _lib.call("umb_logit_softcap", zc, z.numel(), 30.0)
    torch.testing.assert_close(zc, torch.tanh(z / 30.0) * 30.0, rtol=2e-6, atol=2e-6)


@pytest.mark.gpu
def test_qkv_rope_reduce_at_head_dim_256():
    """umb_reduce_qkv_rope (its only shape check is D % 32) at D = 256: q rotated, K / V placed at their slots"""
    from umbrella_amd import _lib
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    T, Hq, Hkv, D, Lmax = 5, 2, 1, 256, 64
    N = (Hq + 2 * Hkv) * D
    part = torch.randn(1, T, N, device=dev)
    pos = torch.tensor([3, 7, 8, 20, 40], dtype=torch.int32, device=dev)
    slot = torch.tensor([0, 1, 2, 33, 63], dtype=torch.int32, device=dev)
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))
    fr = torch.outer(torch.arange(Lmax).float(), inv)
    emb = torch.cat((fr, fr), -1)
    cos, sin = emb.cos().to(dtype).to(dev), emb.sin().to(dtype).to(dev)
    q = torch.empty(T, Hq, D, dtype=dtype, device=dev)
    kc = torch.zeros(Hkv * Lmax * D, dtype=dtype, device=dev)
    vt = torch.zeros(Hkv * D * (Lmax + 32), dtype=dtype, device=dev)
    _lib.call("umb_reduce_qkv_rope", part, 1, T, Hq, Hkv, D, Lmax, pos, slot, cos, sin, q, kc, vt, 0, None,
              _lib.dtype_code(dtype))
    x = part[0].to(dtype).float().view(T, Hq + 2 * Hkv, D)
    c, s_ = cos[pos.long()].float()[:, None], sin[pos.long()].float()[:, None]

    def rot(t):
        r = torch.cat((-t[..., D // 2:], t[..., :D // 2]), -1)
        return ((t * c).to(dtype).float() + (r * s_).to(dtype).float()).to(dtype).float()
    torch.testing.assert_close(q.float(), rot(x[:, :Hq]), rtol=0, atol=0)
    # K / V^T back through the attention kernel's layout: one query per stored key sees exactly that key
    kr, vr = rot(x[:, Hq:Hq + Hkv]), x[:, Hq + Hkv:]
    from umbrella_amd.attn.cache import TreeKVCache  # noqa: F401  (layout owner)
    kd = torch.zeros(Lmax, Hkv, D, dtype=dtype, device=dev)
    vd = torch.zeros(Lmax, Hkv, D, dtype=dtype, device=dev)
    kd[slot.long()] = kr.to(dtype)
    vd[slot.long()] = vr.to(dtype)
    kc2 = torch.zeros_like(kc)
    vt2 = torch.zeros_like(vt)
    _lib.call("umb_kv_append", kc2, vt2, kd, vd, torch.arange(Lmax, dtype=torch.int32, device=dev), Lmax, Hkv, D, Lmax,
              _lib.dtype_code(dtype))
    assert torch.equal(kc, kc2) and torch.equal(vt, vt2)


# ----------------------------------------------------------------------------- GPU: model
@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(gr.CFGS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemma2_logits_vs_fixture(kind, dtype):
    """HIP runtime vs HF's fp32 logits (tolerances of test_hip_family_logits), 40-token prompt across the window;
    offloaded == resident bit for bit"""
    tol, rel = (0.06, 2.0 ** -9) if dtype == torch.float16 else (0.35, 2.0 ** -6)
    outs = []
    for offload in (False, True):
        m = _tiny(kind, dtype, offload=offload)
        logits = _prompt_logits(m, G["prompt"])
        ref = torch.from_numpy(LOG[kind + "_logits"])
        scale = max(1.0, float(ref.abs().max()) / 16.0)
        err = (logits - ref).abs()
        assert (err <= tol * scale + ref.abs() * rel).all(), float(err.max())
        assert (logits.argmax(-1) == ref.argmax(-1)).float().mean() > 0.9
        outs.append(logits)
        del m
    assert torch.equal(outs[0], outs[1])


@pytest.mark.gpu
def test_gemma2_graph_equals_eager():
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
def test_gemma2_out_of_scope_raises():
    from umbrella_amd.models.gemma import Gemma2
    cfg = gr.llama_cfg("A")
    with pytest.raises(NotImplementedError):
        Gemma2("x", device="cuda:0", state_dict=gr.gemma2_state("A"), config=gr.llama_cfg("A", awq=True))
    m = Gemma2("x", device="cuda:0", state_dict=gr.gemma2_state("A"), config=cfg)
    with pytest.raises(NotImplementedError):
        m.alloc(layer_range=(0, 2))
    m = _tiny("A", torch.float16)
    m.use_gemv(True)                                  # no-op
    assert not m.gemv and not getattr(m, "chain", False)


def _engine(kind_t, kind_d, engine, **kw):
    from umbrella_amd.speculation.dynamic_speculation_engine import DynamicSpeculationEngine
    from umbrella_amd.speculation.speculation_utils import IdTokenizer
    from umbrella_amd.speculation.static_speculation_engine import StaticSpeculationEngine
    dtype = torch.float16
    target = _tiny(kind_t, dtype)
    draft = _tiny(kind_d, dtype, cuda_graph=(engine == "static"))
    common = dict(dtype=dtype, device="cuda:0", max_length=256, safe_buffer=16, stop_distance=8, draft_model_obj=draft,
                  target_model_obj=target, tokenizer=IdTokenizer())
    if engine == "static":
        return StaticSpeculationEngine("d", "t", growmap=GM["3x4"], **common)
    return DynamicSpeculationEngine("d", "t", width=kw.get("width", 4), num_beams=kw.get("num_beams", 8),
                                    depth=kw.get("depth", 6), **common)


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["static", "dynamic"])
def test_gemma2_engines_follow_greedy_target(engine):
    """Gemma-2 target (A) and draft (B): every emitted token is an arg-max of the fp32 target within the 16-bit slack, and
    the generation crosses the 16-key window"""
    eng = _engine("A", "B", engine)
    eng.initialize()
    prompt = G["prompt"]
    out = eng.generate(input_ids=prompt, max_new_tokens=48)
    toks = out["generated_tokens"]
    assert len(toks) >= 1
    seq = list(prompt) + toks
    logits = gr.Gemma2Ref("A").forward(seq)
    for i, tok in enumerate(toks):
        row = logits[len(prompt) + i - 1].clone()
        if i == 0 and engine == "dynamic":
            row[[3, 5]] = -float("inf")
        assert float(row.max() - row[tok]) <= 0.1, (i, tok, float(row.max() - row[tok]))
    # and they are HF's greedy tokens up to the first recorded near-tie (margin < 0.1 -- 16-bit arithmetic may take either
    # side there).  Attention decides them: without the window, or with attention zeroed, the first tokens differ.
    hf, margins = G["A_greedy"], G["A_margins"]
    for i in range(min(len(toks), len(hf))):
        if margins[i] < 0.1:
            break
        assert toks[i] == hf[i], (i, toks[:i + 1], hf[:i + 1])


@pytest.mark.gpu
def test_gemma2_engine_rejects_tree_deeper_than_window():
    eng = _engine("A", "B", "dynamic", depth=16)
    with pytest.raises(AssertionError, match="sliding_window"):
        eng.initialize()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["google/gemma-2-2b", "google/gemma-2-9b-it", "google/gemma-2-27b-it"])
def test_gemma2_full_width_two_layers(name):
    """two layers at the published dims (synthetic weights) vs the fp32 restatement on the GPU"""
    import dataclasses
    from umbrella_amd.models.config import KNOWN
    from umbrella_amd.models.gemma import Gemma2
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16
    cfg = dataclasses.replace(KNOWN[name], num_hidden_layers=2, sliding_window=24)
    H, I, Hq, Hkv, D = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    g = torch.Generator(device=dev).manual_seed(5)

    def rn(*shape, s):
        return (torch.randn(*shape, device=dev, generator=g) * s).to(dtype)
    # embedding at std H^-1/2 and heavier post norms (as tests/gemma2_ref.gemma2_state): attention and the MLP, not the
    # token's own tied row, decide the logits
    sd = {"model.embed_tokens.weight": rn(cfg.vocab_size, H, s=H ** -0.5), "model.norm.weight": rn(H, s=0.2) + 3.0}
    shapes = {"self_attn.q_proj": (Hq * D, H), "self_attn.k_proj": (Hkv * D, H), "self_attn.v_proj": (Hkv * D, H),
              "self_attn.o_proj": (H, Hq * D), "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}
    for i in range(2):
        for n, (a, b) in shapes.items():
            sd[f"model.layers.{i}.{n}.weight"] = rn(a, b, s=b ** -0.5)
        for n in ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm"):
            sd[f"model.layers.{i}.{n}.weight"] = rn(H, s=0.2) + (2.0 if n.startswith("post") else 0.0)
    m = Gemma2(name, max_length=256, device=str(dev), dtype=dtype, state_dict=sd, config=cfg)
    m.alloc()
    ids = torch.randint(0, cfg.vocab_size, (50,), generator=torch.Generator().manual_seed(1)).tolist()
    got = _prompt_logits(m, ids)[-8:].to(dev)
    c = dict(vocab_size=cfg.vocab_size, hidden_size=H, intermediate_size=I, num_hidden_layers=2, num_attention_heads=Hq,
             num_key_value_heads=Hkv, head_dim=D, query_pre_attn_scalar=cfg.query_pre_attn_scalar, sliding_window=24,
             **gr.COMMON)
    ref = gr.Gemma2Ref(c, sd).forward(ids)[-8:]
    err = float((got - ref).abs().max())
    # the tolerance must separate a right kernel from a wrong one: the window ignored (50 tokens > 24) or, for the 27B,
    # the scale 1/sqrt(D) instead of query_pre_attn_scalar^-1/2 move the logits several times further than bf16 does
    wrong = [dict(c, sliding_window=0)] + ([dict(c, query_pre_attn_scalar=D)] if c["query_pre_attn_scalar"] != D else [])
    for w in wrong:
        off = float((gr.Gemma2Ref(w, sd).forward(ids)[-8:] - ref).abs().max())
        assert err < 0.3 * off, (err, off, w)
    assert err < 0.5, err
    del m
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_gemma2_27b_target_2b_draft_full_depth(monkeypatch):
    """AutoModelLM.from_pretrained("google/gemma-2-27b-it") end to end with the 2B as draft, synthetic bf16 weights,
    static 3x4: every emitted token is an arg-max of the 27B's own logits over the sequence (within a bf16 tie margin)"""
    from umbrella_amd.models.auto_model import AutoModelLM
    from umbrella_amd.speculation.speculation_utils import IdTokenizer
    from umbrella_amd.speculation.static_speculation_engine import StaticSpeculationEngine
    monkeypatch.setenv("UMBRELLA_SYNTHETIC", "1")
    dtype = torch.bfloat16
    target = AutoModelLM.from_pretrained("google/gemma-2-27b-it", dtype=dtype, max_length=256)
    draft = AutoModelLM.from_pretrained("google/gemma-2-2b-it", dtype=dtype, max_length=256, cuda_graph=True)
    target.alloc()
    draft.alloc()
    eng = StaticSpeculationEngine("google/gemma-2-2b-it", "google/gemma-2-27b-it", growmap=GM["3x4"], dtype=dtype,
                                  device="cuda:0", max_length=256, safe_buffer=16, stop_distance=8, draft_model_obj=draft,
                                  target_model_obj=target, tokenizer=IdTokenizer())
    eng.initialize()
    prompt = torch.randint(1000, 200000, (24,), generator=torch.Generator().manual_seed(2)).tolist()
    out = eng.generate(input_ids=prompt, max_new_tokens=24)
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
