"""FP8 (OCP e4m3fn) weight-only checkpoints, host side: scale shapes, both quantization_config forms, every refusal, packed
sizes, the float64 restatement of the kernel's arithmetic (tests/fp8_ref.py) and tiny FP8 Hugging Face directories in both
naming schemes, read back through safetensors."""
import json
import os

import pytest
import torch

import fp8_ref as fr
from umbrella_amd.models import fp8_format
from umbrella_amd.models.config import KNOWN, LlamaCfg


def test_every_finite_e4m3_code_is_exact_in_fp16_and_bf16():
    codes = fr.finite_codes()
    assert codes.numel() == 254
    v = fr.code_values(codes)
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(v.to(dt).double(), v), dt
    assert float(v.abs().max()) == 448.0 and float(v[v != 0].abs().min()) == 2.0 ** -9


def test_scale_expansion_three_shapes_and_stacked_qkv():
    N, K = 192, 384
    g = torch.Generator().manual_seed(0)
    t = torch.rand(1, generator=g)
    for s in (t, t.reshape(()), t.reshape(1, 1)):
        e = fp8_format.expand_scale(s, N, K)
        assert e.shape == (N, 3) and e.dtype == torch.float32 and bool((e == t.item()).all()) and e.is_contiguous()
    ch = torch.rand(N, 1, generator=g)
    for s in (ch, ch.reshape(N)):
        e = fp8_format.expand_scale(s, N, K)
        assert torch.equal(e, ch.expand(N, 3))
    blk = torch.rand(2, 3, generator=g)                       # ceil(192 / 128) = 2 row blocks, the second one half full
    e = fp8_format.expand_scale(blk, N, K)
    assert e.shape == (N, 3)
    for n in (0, 127, 128, 191):
        assert torch.equal(e[n], blk[n // 128])
    with pytest.raises(ValueError, match="q_proj.weight_scale"):
        fp8_format.expand_scale(torch.rand(5, 3), N, K, "q_proj.weight_scale")
    # q | k | v stacked along N, each part with its own scales (per-tensor parts give per-part constants)
    parts = []
    for i, n in enumerate((256, 128, 128)):
        codes = torch.full((n, K), i, dtype=torch.uint8)
        parts.append((codes, fp8_format.expand_scale(torch.tensor([float(i + 1)]), n, K)))
    codes, rows = fp8_format.stack(parts)
    assert codes.shape == (512, K) and rows.shape == (512, 3)
    assert bool((rows[:256] == 1).all()) and bool((rows[256:384] == 2).all()) and bool((rows[384:] == 3).all())
    assert bool((codes[256:384] == 1).all())


def _write_cfg(tmp_path, kind, q):
    (tmp_path / "config.json").write_text(json.dumps(dict(fr.TINY[kind], quantization_config=q)))
    return str(tmp_path)


def test_both_quantization_config_forms_parse(tmp_path):
    c = LlamaCfg.from_dir(_write_cfg(tmp_path, "qwen3", fr.QUANT_CFG["block128"]))
    assert c.fp8 and c.fp8_scheme == "block128" and not c.awq and c.family == "qwen3"
    for scheme in ("channel", "tensor"):
        c = LlamaCfg.from_dir(_write_cfg(tmp_path, "llama256", fr.QUANT_CFG[scheme]))
        assert c.fp8 and c.fp8_scheme == scheme and not c.awq and c.family == "llama"
    # activation-quantization settings are ignored (weight-only): static and dynamic input scales parse alike
    q = json.loads(json.dumps(fr.QUANT_CFG["channel"]))
    q["config_groups"]["group_0"]["input_activations"] = None
    assert LlamaCfg.from_dir(_write_cfg(tmp_path, "llama256", q)).fp8_scheme == "channel"
    assert LlamaCfg.from_dir(_write_cfg(tmp_path, "llama256", dict(fr.QUANT_CFG["block128"], activation_scheme="static"))).fp8
    # the other formats keep their flags
    c = LlamaCfg.from_dir(_write_cfg(tmp_path, "llama256", {"quant_method": "awq", "group_size": 128}))
    assert c.awq and not c.fp8
    (tmp_path / "config.json").write_text(json.dumps(fr.TINY["llama256"]))
    c = LlamaCfg.from_dir(str(tmp_path))
    assert not c.awq and not c.fp8
    with pytest.raises(ValueError, match="mutually exclusive"):
        LlamaCfg(awq=True, fp8=True)


def test_refused_configs_name_the_offending_key(tmp_path):
    bad = [(dict(fr.QUANT_CFG["block128"], weight_block_size=[64, 64]), "weight_block_size"),
           (dict(fr.QUANT_CFG["block128"], weight_block_size=None), "weight_block_size"),
           (dict(fr.QUANT_CFG["block128"], fmt="e5m2"), "fmt"),
           (dict(fr.QUANT_CFG["block128"], fmt="e4m3fnuz"), "fmt")]
    for strat in ("group", "block"):
        q = json.loads(json.dumps(fr.QUANT_CFG["channel"]))
        q["config_groups"]["group_0"]["weights"]["strategy"] = strat
        bad.append((q, "strategy"))
    q = json.loads(json.dumps(fr.QUANT_CFG["channel"]))
    q["config_groups"]["group_0"]["weights"].update(num_bits=4)
    bad.append((q, "num_bits"))
    q = json.loads(json.dumps(fr.QUANT_CFG["channel"]))
    q["config_groups"]["group_0"]["weights"]["symmetric"] = False
    bad.append((q, "symmetric"))
    for q, key in bad:
        with pytest.raises(ValueError, match=key):
            LlamaCfg.from_dir(_write_cfg(tmp_path, "llama256", q))
    # compressed-tensors builds that are not float (int8, W4A16) are no FP8 checkpoints: parsed as before, no flag, no error
    for bits in (8, 4):
        q = json.loads(json.dumps(fr.QUANT_CFG["channel"]))
        q["config_groups"]["group_0"]["weights"].update(type="int", num_bits=bits)
        c = LlamaCfg.from_dir(_write_cfg(tmp_path, "llama256", q))
        assert not c.fp8 and not c.awq
    assert not LlamaCfg.from_dir(_write_cfg(tmp_path, "llama256", {"quant_method": "compressed-tensors"})).fp8


def test_refused_tensors_name_the_offending_key():
    ok = torch.zeros(64, 128, dtype=torch.float8_e4m3fn)
    assert fp8_format.check_weight("x.weight", ok).dtype == torch.uint8
    with pytest.raises(ValueError, match=r"layers\.0\.mlp\.up_proj\.weight.*e5m2"):
        fp8_format.check_weight("model.layers.0.mlp.up_proj.weight", torch.zeros(64, 128, dtype=torch.float8_e5m2))
    for dt in (torch.float8_e4m3fnuz, torch.float8_e5m2fnuz):
        with pytest.raises(ValueError, match=r"q_proj\.weight.*fnuz"):
            fp8_format.check_weight("q_proj.weight", torch.zeros(64, 128, dtype=dt))
    for code in (0x7F, 0xFF):
        w = torch.zeros(64, 128, dtype=torch.uint8)
        w[17, 5] = code
        with pytest.raises(ValueError, match=r"down_proj\.weight.*NaN"):
            fp8_format.check_weight("down_proj.weight", w.view(torch.float8_e4m3fn))
    w = torch.full((64, 128), 0x7E, dtype=torch.uint8)           # 448, the largest finite value: accepted
    fp8_format.check_weight("w", w.view(torch.float8_e4m3fn))
    # an FP8 lm_head
    with pytest.raises(ValueError, match=r"lm_head\.weight_scale"):
        fp8_format.check_head({"lm_head.weight", "lm_head.weight_scale"}, lambda k: torch.float8_e4m3fn)
    with pytest.raises(ValueError, match=r"lm_head\.weight"):
        fp8_format.check_head({"lm_head.weight"}, lambda k: torch.float8_e4m3fn)
    fp8_format.check_head({"lm_head.weight"}, lambda k: torch.bfloat16)
    fp8_format.check_head({"lm_head.weight"}, lambda k: "BF16")
    with pytest.raises(ValueError, match=r"lm_head\.weight"):
        fp8_format.check_head({"lm_head.weight"}, lambda k: "F8_E4M3")


@pytest.mark.parametrize("how", ["fp8_weight", "scale_tensor"])
def test_loader_refuses_an_fp8_lm_head(tmp_path, how):
    """the loader itself (Llama._tensor_source over the directory's safetensors index) refuses an FP8 head before it
    loads anything; the same directory with a 16-bit head is indexed"""
    from safetensors.torch import save_file
    from umbrella_amd.models.llama import Llama
    path = str(tmp_path)
    stored, _ = fr.write_fp8_dir(path, "llama2048", "channel")          # untied: the directory has its own lm_head.weight
    assert stored["lm_head.weight"].dtype == torch.bfloat16
    fetch = Llama(path, device="cpu")._tensor_source()
    assert callable(fetch)
    if how == "fp8_weight":
        stored["lm_head.weight"] = stored["lm_head.weight"].float().clamp(-448, 448).to(torch.float8_e4m3fn)
        match = r"lm_head\.weight"
    else:
        stored["lm_head.weight_scale"] = torch.ones(1)
        match = r"lm_head\.weight_scale"
    save_file({k: t.contiguous() for k, t in stored.items()}, os.path.join(path, "model.safetensors"))
    with pytest.raises(ValueError, match=match):
        Llama(path, device="cpu")._tensor_source()


def test_packed_bytes_format_2_and_registry():
    from umbrella_amd.models.auto_model import AutoModelLM
    from umbrella_amd.models.llama import Llama, PackedLinear
    from umbrella_amd.models.qwen3 import Qwen3
    assert PackedLinear.packed_bytes(10240, 8192, 2) == (10240 * 8192, (10240 // 16) * 64 * 64)
    assert PackedLinear.packed_bytes(64, 128, 2) == (8192, 256)
    assert PackedLinear.raw_bytes(192, 384, 2) == (192 * 384, 12 * 3 * 64)
    # the older formats keep their sizes (bool or code)
    assert PackedLinear.packed_bytes(64, 128, True) == PackedLinear.packed_bytes(64, 128, 1) == (4096, 256)
    assert PackedLinear.packed_bytes(64, 128, False) == PackedLinear.packed_bytes(64, 128, 0) == (16384, 0)
    for size in ("0.6B", "1.7B", "4B", "8B", "14B", "32B"):
        c, d = KNOWN[f"Qwen/Qwen3-{size}-FP8"], KNOWN[f"Qwen/Qwen3-{size}"]
        assert c.fp8 and c.fp8_scheme == "block128" and not c.awq and c.family == "qwen3"
        assert (c.hidden_size, c.intermediate_size, c.num_hidden_layers) == (d.hidden_size, d.intermediate_size, d.num_hidden_layers)
        assert AutoModelLM._MODEL_MAPPING[f"Qwen/Qwen3-{size}-FP8"] is Qwen3
    fp8_llamas = [k for k, c in KNOWN.items() if c.fp8 and c.family == "llama"]
    assert len(fp8_llamas) == 3
    for k in fp8_llamas:
        assert KNOWN[k].hidden_size in (4096, 8192) and AutoModelLM._MODEL_MAPPING[k] is Llama
    m = AutoModelLM.from_pretrained("Qwen/Qwen3-32B-FP8", max_length=64)
    assert m.sched == "split" and not m.fused
    m = Llama(fp8_llamas[0], max_length=64, sched="ll")
    assert m.sched == "split" and not m.fused


def test_fp8_never_reaches_a_runtime_without_it():
    from umbrella_amd.models.gemma import Gemma2
    from umbrella_amd.models.llama import Llama
    from umbrella_amd.parallel import build_pipelined_engine
    name = "Qwen/Qwen3-32B-FP8"
    lname = next(k for k, c in KNOWN.items() if c.fp8 and c.family == "llama")
    with pytest.raises(NotImplementedError, match="offload"):
        Llama(lname, offload=True)
    with pytest.raises(NotImplementedError):
        build_pipelined_engine("cpu", model=lname, draft_model="meta-llama/Llama-3.2-1B-Instruct", engine="static")
    # tensor parallelism: the builder and the wrapper; layer pipelining through alloc(layer_range=...)
    from types import SimpleNamespace
    from umbrella_amd.tensor_parallel import TensorParallelLlama, build_tp_engine
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        TensorParallelLlama.build(KNOWN[lname], {}, None, 256, "cpu", torch.bfloat16)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        TensorParallelLlama(KNOWN[lname], SimpleNamespace(config=KNOWN[lname]), None)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        build_tp_engine("cpu", model=lname, draft_model="meta-llama/Llama-3.2-1B-Instruct", engine="static")
    with pytest.raises(NotImplementedError, match="layer pipelining"):
        Llama(lname, device="cpu").alloc(layer_range=(0, 2))
    m = Llama(lname, device="cpu")
    m._tp = object()
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        m.alloc()
    import dataclasses
    with pytest.raises(NotImplementedError):
        Gemma2("x", config=dataclasses.replace(KNOWN["google/gemma-2-2b"], fp8=True, fp8_scheme="channel"))
    assert KNOWN[name].fp8


def test_restatement_against_dequantised_matmul():
    """tests/fp8_ref.gemm_ref (float64, the kernel's grouping) against (w8.float() * scale) @ x on random data: equal to
    fp32 rounding of the reference product"""
    g = torch.Generator().manual_seed(4)
    N, K, T = 64, 384, 5
    codes = fr.finite_codes()[torch.randint(0, 254, (N, K), generator=g)]
    rows = torch.rand(N, K // 128, generator=g) * 0.01 + 0.001
    x = torch.randn(T, K, generator=g).to(torch.bfloat16)
    for S in (1, 2, 3, 5):
        ref = fr.gemm_ref(codes, rows, x, S)
        assert ref.shape == (S, T, N)
        if S == 5:
            assert bool((ref[3:] == 0).all())                  # K / 128 = 3: per = 1, slabs 3 and 4 are empty
        w = fp8_format.dequant(codes, rows)                    # fp32, one rounding per weight
        want = x.float() @ w.t()
        err = (ref.sum(0) - want.double()).abs()
        bound = (x.float().abs() @ w.abs().t()).double() * (K + 2) * 2.0 ** -24
        assert bool((err <= bound).all()), float((err / bound).max())


def test_integer_operands_keep_the_restatement_exact():
    """the bit-for-bit GPU cases: on fp8_ref.int_operands every partial sum of the restatement is a fp32 value and |G_g| < 2^24,
    so fp32 accumulation in ANY order gives exactly the float64 result"""
    for (N, K, T) in ((64, 128, 3), (192, 384, 17), (64, 1024, 64)):
        for dtype in (torch.float16, torch.bfloat16):
            codes, rows, x = fr.int_operands(N, K, T, seed=N + K + T, dtype=dtype)
            assert float(fr.code_values(codes).abs().max()) <= 8 and float(x.float().abs().max()) <= 4
            assert torch.equal(x.float().double(), x.double())
            for S in (1, 2, 3, 5):
                ref = fr.gemm_ref(codes, rows, x, S)
                assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) < 2.0 ** 24
            # worst case over any operands of these ranges, not only the drawn ones
            assert K * 8 * 4 * 8 < 2 ** 24 and 128 * 8 * 4 <= 2 ** 12


@pytest.mark.parametrize("kind,scheme", [("llama256", "channel"), ("llama256", "tensor"), ("qwen3", "block128"),
                                         ("qwen2", "block128")])
def test_tiny_fp8_directory_round_trip(tmp_path, kind, scheme):
    """a 2-layer H 256 FP8 directory in either naming scheme: safetensors stores float8_e4m3fn, the config parses, every
    projection passes the checks and its expanded scales reproduce the oracle's dense weight"""
    from safetensors import safe_open
    stored, dense = fr.write_fp8_dir(str(tmp_path), kind, scheme)
    c = LlamaCfg.from_dir(str(tmp_path))
    assert c.fp8 and c.fp8_scheme == scheme and c.hidden_size == 256 and c.num_hidden_layers == 2
    assert c.attention_bias == (kind == "qwen2")
    suffix = fp8_format.SCALE_SUFFIX[scheme]
    assert suffix == (".weight_scale_inv" if scheme == "block128" else ".weight_scale")
    with safe_open(os.path.join(str(tmp_path), "model.safetensors"), "pt") as h:
        keys = set(h.keys())
        fp8_format.check_head(keys, lambda k: h.get_tensor(k).dtype)
        n = 0
        for k in sorted(keys):
            if not k.endswith("_proj.weight"):
                assert h.get_tensor(k).dtype == torch.bfloat16 or k.endswith(suffix), k
                continue
            w = h.get_tensor(k)
            assert w.dtype == torch.float8_e4m3fn
            codes = fp8_format.check_weight(k, w)
            s = h.get_tensor(k[:-len(".weight")] + suffix)
            assert s.dtype == torch.float32
            assert tuple(s.shape) == {"block128": ((w.shape[0] + 127) // 128, w.shape[1] // 128), "channel": (w.shape[0], 1),
                                      "tensor": (1,)}[scheme]
            rows = fp8_format.expand_scale(s, *w.shape, k + suffix)
            assert torch.equal(fp8_format.dequant(codes, rows), dense[k])
            # quantisation error of the fixture itself: e4m3 keeps 3 mantissa bits
            full = fr.tiny_state(kind)[k]
            assert float((dense[k] - full).abs().max()) <= float(full.abs().max()) * 2.0 ** -4
            n += 1
        assert n == 14
