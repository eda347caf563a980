"""Test-side restatements for the FP8 (e4m3, weight-only) linears: the arithmetic of record in float64, the table of finite
codes, exact-integer operand makers and tiny FP8 Hugging Face directories in both naming schemes (tests only)."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from umbrella_amd.models import fp8_format

GROUP = 128


def finite_codes() -> torch.Tensor:
    """the 254 non-NaN e4m3fn codes (uint8), +-0 and the subnormals included"""
    b = torch.arange(256, dtype=torch.int32)
    return b[(b & 0x7F) != 0x7F].to(torch.uint8)


def code_values(codes: torch.Tensor) -> torch.Tensor:
    """uint8 codes -> their real values (float64), through torch's float8_e4m3fn"""
    return codes.contiguous().view(torch.float8_e4m3fn).to(torch.float64)


def gemm_ref(codes: torch.Tensor, scale_rows: torch.Tensor, x: torch.Tensor, S: int = 1) -> torch.Tensor:
    """The arithmetic of record in float64: out[s][t][n] = sum over the slab's 128-k groups g (ascending) of
    scale[n][g] * G_g,  G_g = sum_k value(codes[n][k]) * x[t][k] over group g.  Slab s covers the groups
    [s * per, min(K/128, (s + 1) * per)), per = ceil((K/128) / S); an empty slab is zeros.  Returns [S][T][N] float64."""
    N, K = codes.shape
    T = x.shape[0]
    KG = K // GROUP
    w = code_values(codes.cpu()).view(N, KG, GROUP)
    xs = x.detach().cpu().to(torch.float64).view(T, KG, GROUP)
    sc = scale_rows.detach().cpu().to(torch.float64)
    per = (KG + S - 1) // S
    out = torch.zeros(S, T, N, dtype=torch.float64)
    for s in range(S):
        for g in range(s * per, min(KG, (s + 1) * per)):
            G = xs[:, g, :] @ w[:, g, :].t()                  # [T][N]
            out[s] = sc[:, g][None, :] * G + out[s]
    return out


def int_operands(N: int, K: int, T: int, seed: int, dtype=torch.float16):
    """Operands on which fp32 accumulation is exact in any order: codes of integers |w| <= 8, integer activations |x| <= 4,
    power-of-two scales 2^-3 .. 2^3.  |G_g| <= 128 * 32 = 2^12 and |out| <= K * 32 * 8 < 2^24 at K <= 1024, every partial
    sum a multiple of 2^-3: all exactly representable in fp32.  Returns (codes uint8 [N][K], scale_rows fp32, x dtype [T][K])."""
    g = torch.Generator().manual_seed(seed)
    wi = torch.randint(-8, 9, (N, K), generator=g).to(torch.float32)
    codes = wi.to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(code_values(codes), wi.double())
    scale = torch.pow(2.0, torch.randint(-3, 4, (N, K // GROUP), generator=g).float())
    x = torch.randint(-4, 5, (T, K), generator=g).to(dtype)
    return codes, scale, x


def rowmap(n: int, N: int, mode: int, D: int, rope_heads: int) -> int:
    """packed row n <- source row (csrc/gemm.hip rowmap)"""
    if mode == 1:
        return N // 2 + (n >> 1) if n & 1 else n >> 1
    if mode == 2:
        head, dp = divmod(n, D)
        if head >= rope_heads:
            return n
        return head * D + ((dp >> 1) + D // 2 if dp & 1 else dp >> 1)
    return n


# ----------------------------------------------------------------------------- tiny FP8 checkpoints on disk
TINY = {
    # H 256: the in-place norm layer (H % 2048 != 0)
    "llama256": dict(model_type="llama", vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                     num_attention_heads=4, num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-5, rope_theta=10000.0,
                     max_position_embeddings=2048, tie_word_embeddings=True, eos_token_id=[3, 5]),
    # H 2048: the deferred-norm layer (csrc/model.hip use_defer wants H % 2048 == 0)
    "llama2048": dict(model_type="llama", vocab_size=512, hidden_size=2048, intermediate_size=1024, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2, head_dim=64, rms_norm_eps=1e-5, rope_theta=10000.0,
                      max_position_embeddings=2048, tie_word_embeddings=False, eos_token_id=[3, 5]),
    # Qwen2-style q/k/v bias
    "qwen2": dict(model_type="qwen2", vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                  num_attention_heads=4, num_key_value_heads=2, rms_norm_eps=1e-6, rope_theta=10000.0,
                  max_position_embeddings=2048, tie_word_embeddings=True, eos_token_id=[3, 5]),
    "qwen3": dict(model_type="qwen3", vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                  num_attention_heads=4, num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-6, rope_theta=1000000.0,
                  max_position_embeddings=40960, tie_word_embeddings=True, attention_bias=False, eos_token_id=[3, 5]),
    # Qwen3 on the deferred-norm layer
    "qwen3_2048": dict(model_type="qwen3", vocab_size=512, hidden_size=2048, intermediate_size=1024, num_hidden_layers=2,
                       num_attention_heads=4, num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-6, rope_theta=1000000.0,
                       max_position_embeddings=40960, tie_word_embeddings=True, attention_bias=False, eos_token_id=[3, 5]),
}
QUANT_CFG = {
    "block128": {"quant_method": "fp8", "fmt": "e4m3", "activation_scheme": "dynamic", "weight_block_size": [128, 128]},
    "channel": {"quant_method": "compressed-tensors", "format": "float-quantized", "config_groups": {"group_0": {
        "targets": ["Linear"], "weights": {"type": "float", "num_bits": 8, "symmetric": True, "strategy": "channel",
                                           "dynamic": False},
        "input_activations": {"type": "float", "num_bits": 8, "symmetric": True, "strategy": "token", "dynamic": True}}},
        "ignore": ["lm_head"]},
    "tensor": {"quant_method": "compressed-tensors", "format": "float-quantized", "config_groups": {"group_0": {
        "targets": ["Linear"], "weights": {"type": "float", "num_bits": 8, "symmetric": True, "strategy": "tensor",
                                           "dynamic": False},
        "input_activations": {"type": "float", "num_bits": 8, "symmetric": True, "strategy": "tensor", "dynamic": False}}},
        "ignore": ["lm_head"]},
}


def tiny_state(kind: str, seed: int = 11) -> dict:
    """fp32 HF-named dense state dict of a TINY config (numpy-seeded): linears N(0, 1/fan_in), norms around 1"""
    c = TINY[kind]
    rs = np.random.RandomState(seed)
    H, I, Hq, Hkv = c["hidden_size"], c["intermediate_size"], c["num_attention_heads"], c["num_key_value_heads"]
    D = c.get("head_dim") or H // Hq

    def nrm(*shape, s):
        return torch.from_numpy((rs.standard_normal(shape) * s).astype(np.float32))
    shapes = {"self_attn.q_proj": (Hq * D, H), "self_attn.k_proj": (Hkv * D, H), "self_attn.v_proj": (Hkv * D, H),
              "self_attn.o_proj": (H, Hq * D), "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}
    sd = {"model.embed_tokens.weight": nrm(c["vocab_size"], H, s=0.25)}
    for i in range(c["num_hidden_layers"]):
        p = f"model.layers.{i}."
        for n, (a, b) in shapes.items():
            sd[p + n + ".weight"] = nrm(a, b, s=(2.0 if n.endswith("o_proj") else 1.0) / np.sqrt(b))
        for n in ("input_layernorm", "post_attention_layernorm"):
            sd[p + n + ".weight"] = nrm(H, s=0.1) + 1.0
        if c["model_type"] == "qwen3":
            sd[p + "self_attn.q_norm.weight"] = nrm(D, s=0.2) + 1.3
            sd[p + "self_attn.k_norm.weight"] = nrm(D, s=0.2) + 1.2
        if c["model_type"] == "qwen2":
            for n in ("q_proj", "k_proj", "v_proj"):
                sd[p + f"self_attn.{n}.bias"] = nrm(shapes["self_attn." + n][0], s=0.3)
    sd["model.norm.weight"] = nrm(H, s=0.1) + 1.5
    if not c["tie_word_embeddings"]:
        sd["lm_head.weight"] = nrm(c["vocab_size"], H, s=0.3)
    return sd


def write_fp8_dir(path: str, kind: str, scheme: str, seed: int = 11, dtype=torch.bfloat16):
    """Write a tiny FP8 Hugging Face directory (config.json + model.safetensors) in the naming scheme of ``scheme``:
    every *_proj.weight as float8_e4m3fn with its *.weight_scale_inv (block128) or *.weight_scale (channel [N, 1] /
    tensor [1]); everything else in ``dtype``.  Returns (the stored tensors, the fp32 dense state an oracle computes with:
    value(weight) * scale for the linears, the stored 16-bit values for the rest)."""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    sd = tiny_state(kind, seed)
    stored, dense = {}, {}
    for k, v in sd.items():
        if k.endswith("_proj.weight"):
            q, s = fp8_format.quantize(v, scheme)
            base = k[:-len(".weight")]
            stored[k] = q
            stored[base + fp8_format.SCALE_SUFFIX[scheme]] = s
            rows = fp8_format.expand_scale(s, v.shape[0], v.shape[1])
            dense[k] = fp8_format.dequant(q.view(torch.uint8), rows)
        else:
            stored[k] = v.to(dtype)
            dense[k] = stored[k].float()
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(TINY[kind], quantization_config=QUANT_CFG[scheme]), f)
    save_file({k: t.contiguous() for k, t in stored.items()}, os.path.join(path, "model.safetensors"))
    return stored, dense
