"""Llama architecture descriptors and RoPE frequency tables.

The reference resolves models by exact hub id through three dicts
(umbrella/models/auto_model.py:9-182) and reads dims from
``LlamaConfig.from_pretrained`` (umbrella/models/llama.py:24-33).  This box has
no hub access, so the public dims of the BASELINE models are tabulated here;
a local directory holding ``config.json`` is accepted as well.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass, field
from typing import Optional

import torch

LLAMA3_ROPE = {"rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0,
               "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}
LLAMA31_ROPE = dict(LLAMA3_ROPE, factor=8.0)


@dataclass
class LlamaCfg:
    vocab_size: int = 128256
    hidden_size: int = 2048
    intermediate_size: int = 8192
    num_hidden_layers: int = 16
    num_attention_heads: int = 32
    num_key_value_heads: int = 8
    head_dim: int = 64
    rms_norm_eps: float = 1e-5
    rope_theta: float = 500000.0
    rope_scaling: Optional[dict] = None
    max_position_embeddings: int = 131072
    tie_word_embeddings: bool = False
    eos_token_id: list = field(default_factory=lambda: [128001, 128008, 128009])
    awq: bool = False                 # 4-bit AWQ (GEMM format, group 128, zero point)
    awq_group: int = 128
    fp8: bool = False                 # FP8 e4m3 weight-only linears (W8A16; models/fp8_format.py); never together with awq
    fp8_scheme: str = ""              # "block128" (*.weight_scale_inv) | "tensor" | "channel" (*.weight_scale)
    name: str = "llama"
    attention_bias: bool = False      # q/k/v projection bias (Qwen2: umbrella/models/qwen.py:94-96)
    embed_rows: int = 0               # rows of the embedding table when they differ from vocab_size (tensor-parallel shard:
                                      # the table stays whole while the lm_head holds vocab_size = V / P rows); 0 = vocab_size
    # Gemma-2 (umbrella/models/gemma.py); the defaults are "off" and leave every other family as it was
    family: str = "llama"             # "gemma2": models/gemma.py Gemma2 runtime; "qwen3": models/qwen3.py Qwen3 runtime
    attn_logit_softcapping: float = 0.0    # scores -> cap * tanh(scores / cap); 0 = off
    final_logit_softcapping: float = 0.0   # logits -> cap * tanh(logits / cap); 0 = off
    query_pre_attn_scalar: float = 0.0     # attention scale query_pre_attn_scalar ** -0.5; 0 = head_dim
    sliding_window: int = 0           # keys a sliding layer sees (p - c < window); 0 = every layer global
    sliding_parity: int = 0           # layer l slides when l % 2 == sliding_parity (Gemma-2: the even layers)
    hidden_activation: str = "silu"   # MLP gate: "silu" or "gelu_pytorch_tanh"

    def __post_init__(self):
        if self.awq and self.fp8:
            raise ValueError(f"'{self.name}': awq and fp8 are mutually exclusive weight formats")

    @property
    def q_dim(self):
        return self.num_attention_heads * self.head_dim

    @property
    def kv_dim(self):
        return self.num_key_value_heads * self.head_dim

    @property
    def attn_scale(self) -> float:
        return (self.query_pre_attn_scalar or self.head_dim) ** -0.5

    def is_sliding(self, layer: int) -> bool:
        return self.sliding_window > 0 and layer % 2 == self.sliding_parity

    @classmethod
    def from_dir(cls, path: str) -> "LlamaCfg":
        with open(os.path.join(path, "config.json")) as f:
            c = json.load(f)
        rp = c.get("rope_parameters") or {}
        rs = c.get("rope_scaling") or ({k: v for k, v in rp.items() if k != "rope_theta"} if rp.get("rope_type", "default") != "default" else None)
        eos = c.get("eos_token_id", 2)
        gen = os.path.join(path, "generation_config.json")
        if os.path.exists(gen):                     # engines read eos from GenerationConfig (static:104-108)
            with open(gen) as f:
                eos = json.load(f).get("eos_token_id", eos)
        q = c.get("quantization_config") or {}
        from .fp8_format import parse_quant_config
        fp8_scheme = parse_quant_config(q)          # None: not an FP8 checkpoint; ValueError: an FP8 form that is not computed
        if c.get("model_type") == "gemma2":
            if fp8_scheme:
                raise NotImplementedError("FP8 checkpoints are not supported for Gemma-2 (quantization_config.quant_method = "
                                          f"{q.get('quant_method')!r})")
            return cls._gemma2_from_dict(c, eos, q, path)
        if c.get("model_type") == "qwen3_moe":
            raise NotImplementedError("Qwen3-MoE (model_type 'qwen3_moe') is not supported: dense Qwen3 only")
        family = "llama"
        if c.get("model_type") == "qwen3":         # HF Qwen3Config: per-head q/k RMSNorm (models/qwen3.py)
            family = "qwen3"
            if c.get("use_sliding_window") or any(t != "full_attention" for t in (c.get("layer_types") or [])):
                raise NotImplementedError("Qwen3 with sliding-window attention layers is not supported "
                                          f"(use_sliding_window={c.get('use_sliding_window')}, layer_types={c.get('layer_types')})")
        qwen = c.get("model_type") == "qwen2"
        if qwen:                                    # the reference pins Qwen2.5's vocabulary (qwen.py:12,27)
            c["vocab_size"] = min(c["vocab_size"], 151936)
        return cls(family=family, attention_bias=bool(c.get("attention_bias", qwen)), vocab_size=c["vocab_size"],
                   hidden_size=c["hidden_size"],
                   intermediate_size=c["intermediate_size"], num_hidden_layers=c["num_hidden_layers"],
                   num_attention_heads=c["num_attention_heads"],
                   num_key_value_heads=c.get("num_key_value_heads", c["num_attention_heads"]),
                   head_dim=c.get("head_dim") or c["hidden_size"] // c["num_attention_heads"],
                   rms_norm_eps=c.get("rms_norm_eps", 1e-6),
                   rope_theta=c.get("rope_theta") or rp.get("rope_theta", 10000.0), rope_scaling=rs,
                   max_position_embeddings=c.get("max_position_embeddings", 8192),
                   tie_word_embeddings=c.get("tie_word_embeddings", False),
                   eos_token_id=eos if isinstance(eos, list) else [eos],
                   awq=q.get("quant_method") == "awq", awq_group=q.get("group_size", 128),
                   fp8=bool(fp8_scheme), fp8_scheme=fp8_scheme or "",
                   name=os.path.basename(os.path.normpath(path)))

    @classmethod
    def _gemma2_from_dict(cls, c: dict, eos, q: dict, path: str) -> "LlamaCfg":
        """HF Gemma2Config (config.json of model_type "gemma2"): layer_types, when present, must alternate sliding / full."""
        rp = c.get("rope_parameters") or {}
        lt = c.get("layer_types")
        parity = 0
        if lt:
            slide = [t == "sliding_attention" for t in lt]
            parity = 0 if slide[0] else 1
            if any(s != ((i % 2) == parity) for i, s in enumerate(slide)):
                raise NotImplementedError(f"Gemma-2 layer_types must alternate sliding / full attention, got {lt}")
        H, Hq = c["hidden_size"], c["num_attention_heads"]
        D = c.get("head_dim") or H // Hq
        return cls(family="gemma2", vocab_size=c["vocab_size"], hidden_size=H, intermediate_size=c["intermediate_size"],
                   num_hidden_layers=c["num_hidden_layers"], num_attention_heads=Hq,
                   num_key_value_heads=c.get("num_key_value_heads", Hq), head_dim=D,
                   rms_norm_eps=c.get("rms_norm_eps", 1e-6), rope_theta=c.get("rope_theta") or rp.get("rope_theta", 10000.0),
                   rope_scaling=None, max_position_embeddings=c.get("max_position_embeddings", 8192),
                   tie_word_embeddings=c.get("tie_word_embeddings", True),
                   eos_token_id=eos if isinstance(eos, list) else [eos], awq=q.get("quant_method") == "awq",
                   # missing keys take HF Gemma2Config's defaults; an explicit null turns the feature off
                   attn_logit_softcapping=float(c.get("attn_logit_softcapping", 50.0) or 0.0),
                   final_logit_softcapping=float(c.get("final_logit_softcapping", 30.0) or 0.0),
                   query_pre_attn_scalar=float(c.get("query_pre_attn_scalar", 256) or D),
                   sliding_window=int(c.get("sliding_window", 4096) or 0), sliding_parity=parity,
                   hidden_activation=c.get("hidden_activation") or c.get("hidden_act") or "gelu_pytorch_tanh",
                   name=os.path.basename(os.path.normpath(path)))


def require_family(cfg: LlamaCfg, family: str, what: str) -> None:
    """Runtimes are per family: a Gemma-2 config on the Llama kernels would run SiLU, Llama norms and 1/sqrt(D) silently."""
    if cfg.family != family:
        raise NotImplementedError(f"{what} runs {family} models only; '{cfg.name}' is a {cfg.family} model"
                                  + (" (models/gemma.py Gemma2: single GPU, resident or offloaded)" if cfg.family == "gemma2" else "")
                                  + (" (models/qwen3.py Qwen3: single GPU, resident or offloaded)" if cfg.family == "qwen3" else ""))


def _l(**kw):
    return LlamaCfg(**kw)


# Public HF configs of the hub ids the reference registers for Llama
# (auto_model.py:9-154) and that BASELINE.json's configs name.
KNOWN = {
    "meta-llama/Llama-3.2-1B-Instruct": _l(hidden_size=2048, intermediate_size=8192, num_hidden_layers=16,
        num_attention_heads=32, num_key_value_heads=8, head_dim=64, rope_scaling=LLAMA3_ROPE,
        tie_word_embeddings=True, name="llama-3.2-1b"),
    "meta-llama/Llama-3.1-8B-Instruct": _l(hidden_size=4096, intermediate_size=14336, num_hidden_layers=32,
        num_attention_heads=32, num_key_value_heads=8, head_dim=128, rope_scaling=LLAMA31_ROPE, name="llama-3.1-8b"),
    "hugging-quants/Meta-Llama-3.1-8B-Instruct-AWQ-INT4": _l(hidden_size=4096, intermediate_size=14336,
        num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=8, head_dim=128,
        rope_scaling=LLAMA31_ROPE, awq=True, name="llama-3.1-8b-awq"),
    "hugging-quants/Meta-Llama-3.1-70B-Instruct-AWQ-INT4": _l(hidden_size=8192, intermediate_size=28672,
        num_hidden_layers=80, num_attention_heads=64, num_key_value_heads=8, head_dim=128,
        rope_scaling=LLAMA31_ROPE, awq=True, name="llama-3.1-70b-awq"),
    "casperhansen/llama-3.3-70b-instruct-awq": _l(hidden_size=8192, intermediate_size=28672,
        num_hidden_layers=80, num_attention_heads=64, num_key_value_heads=8, head_dim=128,
        rope_scaling=LLAMA31_ROPE, awq=True, name="llama-3.3-70b-awq"),
}


def _qwen(H, I, L, Hq, Hkv, tie, awq=False, name="qwen2.5"):
    return LlamaCfg(vocab_size=151936, hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=Hq,
                    num_key_value_heads=Hkv, head_dim=128 if H != 896 else 64, rms_norm_eps=1e-6, rope_theta=1000000.0,
                    rope_scaling=None, max_position_embeddings=32768, tie_word_embeddings=tie,
                    eos_token_id=[151645, 151643], awq=awq, attention_bias=True, name=name)


# Qwen2.5 / Mistral families the reference registers (auto_model.py:21-55, 80-154): public HF dims.
_QWEN_DIMS = {"0.5B": (896, 4864, 24, 14, 2, True), "1.5B": (1536, 8960, 28, 12, 2, True),
              "3B": (2048, 11008, 36, 16, 2, True), "7B": (3584, 18944, 28, 28, 4, False),
              "14B": (5120, 13824, 48, 40, 8, False), "32B": (5120, 27648, 64, 40, 8, False),
              "72B": (8192, 29568, 80, 64, 8, False)}
for _size, _d in _QWEN_DIMS.items():
    for _stem in ("Qwen/Qwen2.5-", "Qwen/Qwen2.5-Coder-"):
        KNOWN[f"{_stem}{_size}-Instruct"] = _qwen(*_d, name=f"qwen2.5-{_size.lower()}")
        KNOWN[f"{_stem}{_size}-Instruct-AWQ"] = _qwen(*_d, awq=True, name=f"qwen2.5-{_size.lower()}-awq")
KNOWN["Qwen/QwQ-32B-Preview"] = _qwen(*_QWEN_DIMS["32B"], name="qwq-32b")
KNOWN["KirillR/QwQ-32B-Preview-AWQ"] = _qwen(*_QWEN_DIMS["32B"], awq=True, name="qwq-32b-awq")
KNOWN["casperhansen/deepseek-r1-distill-qwen-32b-awq"] = _qwen(*_QWEN_DIMS["32B"], awq=True, name="r1-distill-qwen-32b-awq")


def _mistral(V, H, I, L, theta, awq=False, name="mistral"):
    return LlamaCfg(vocab_size=V, hidden_size=H, intermediate_size=I, num_hidden_layers=L, num_attention_heads=32,
                    num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-5, rope_theta=theta, rope_scaling=None,
                    max_position_embeddings=32768, tie_word_embeddings=False, eos_token_id=[2], awq=awq, name=name)


KNOWN["mistralai/Mistral-7B-Instruct-v0.3"] = _mistral(32768, 4096, 14336, 32, 1000000.0, name="mistral-7b-v0.3")
KNOWN["solidrust/Mistral-7B-Instruct-v0.3-AWQ"] = _mistral(32768, 4096, 14336, 32, 1000000.0, awq=True, name="mistral-7b-v0.3-awq")
# head_dim 128 with hidden 5120: attention width Hq*D = 4096 != hidden (mistral.py:28,101)
KNOWN["mistralai/Mistral-Small-24B-Instruct-2501"] = _mistral(131072, 5120, 32768, 40, 100000000.0, name="mistral-small-24b")
KNOWN["stelterlab/Mistral-Small-24B-Instruct-2501-AWQ"] = _mistral(131072, 5120, 32768, 40, 100000000.0, awq=True, name="mistral-small-24b-awq")
# further Llama-family ids of the reference registry (auto_model.py:9-20,58-79) with public dims
_L70 = dict(hidden_size=8192, intermediate_size=28672, num_hidden_layers=80, num_attention_heads=64, num_key_value_heads=8,
            head_dim=128)
_L8 = dict(hidden_size=4096, intermediate_size=14336, num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=8,
           head_dim=128)
for _name in ("ibnzterrell/Meta-Llama-3.3-70B-Instruct-AWQ-INT4", "lambdalabs/Llama-3.3-70B-Instruct-AWQ-4bit",
              "casperhansen/deepseek-r1-distill-llama-70b-awq"):
    KNOWN[_name] = _l(**_L70, rope_scaling=LLAMA31_ROPE, awq=True, name="llama-70b-awq")
for _name in ("meta-llama/Llama-3.3-70B-Instruct", "meta-llama/Llama-3.1-70B-Instruct"):
    KNOWN[_name] = _l(**_L70, rope_scaling=LLAMA31_ROPE, name="llama-3.x-70b")
# Llama 3 (8k context, no rope scaling, eos = <|end_of_text|>, <|eot_id|>)
KNOWN["meta-llama/Meta-Llama-3-70B-Instruct"] = _l(**_L70, max_position_embeddings=8192, eos_token_id=[128001, 128009],
                                                    name="llama-3-70b")
KNOWN["meta-llama/Meta-Llama-3-8B-Instruct"] = _l(**_L8, max_position_embeddings=8192, eos_token_id=[128001, 128009],
                                                   name="llama-3-8b")
KNOWN["meta-llama/Llama-3.2-3B-Instruct"] = _l(hidden_size=3072, intermediate_size=8192, num_hidden_layers=28,
    num_attention_heads=24, num_key_value_heads=8, head_dim=128, rope_scaling=LLAMA3_ROPE, tie_word_embeddings=True,
    name="llama-3.2-3b")
KNOWN["facebook/layerskip-llama3.2-1B"] = KNOWN["meta-llama/Llama-3.2-1B-Instruct"]
KNOWN["Felladrin/Llama-68M-Chat-v1"] = _l(vocab_size=32000, hidden_size=768, intermediate_size=3072, num_hidden_layers=2,
    num_attention_heads=12, num_key_value_heads=12, head_dim=64, rms_norm_eps=1e-6, rope_theta=10000.0,
    max_position_embeddings=2048, eos_token_id=[2], name="llama-68m")
# The reference's small code drafters (Zhuominc/*, InfiniAILab/CodeDrafter-500M) publish no dims here: pass a local
# directory with config.json for those.
KNOWN["meta-llama/Llama-3.2-1B"] = KNOWN["meta-llama/Llama-3.2-1B-Instruct"]
KNOWN["meta-llama/Meta-Llama-3.1-8B-Instruct"] = KNOWN["meta-llama/Llama-3.1-8B-Instruct"]



def _gemma2(H, I, L, Hq, Hkv, D, qpas, name):
    return LlamaCfg(family="gemma2", vocab_size=256000, hidden_size=H, intermediate_size=I, num_hidden_layers=L,
                    num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, rms_norm_eps=1e-6, rope_theta=10000.0,
                    rope_scaling=None, max_position_embeddings=8192, tie_word_embeddings=True, eos_token_id=[1, 107],
                    attn_logit_softcapping=50.0, final_logit_softcapping=30.0, query_pre_attn_scalar=float(qpas),
                    sliding_window=4096, sliding_parity=0, hidden_activation="gelu_pytorch_tanh", name=name)


# Gemma-2 ids the reference maps to its Gemma2 class (auto_model.py:111-114): public HF dims
KNOWN["google/gemma-2-2b"] = _gemma2(2304, 9216, 26, 8, 4, 256, 256, "gemma-2-2b")
KNOWN["google/gemma-2-2b-it"] = _gemma2(2304, 9216, 26, 8, 4, 256, 256, "gemma-2-2b-it")
KNOWN["google/gemma-2-9b-it"] = _gemma2(3584, 14336, 42, 16, 8, 256, 256, "gemma-2-9b-it")
KNOWN["google/gemma-2-27b-it"] = _gemma2(4608, 36864, 46, 32, 16, 128, 144, "gemma-2-27b-it")


def _qwen3(H, I, L, Hq, Hkv, tie, awq=False, name="qwen3", fp8=False):
    return LlamaCfg(family="qwen3", vocab_size=151936, hidden_size=H, intermediate_size=I, num_hidden_layers=L,
                    num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=128, rms_norm_eps=1e-6, rope_theta=1000000.0,
                    rope_scaling=None, max_position_embeddings=40960, tie_word_embeddings=tie,
                    eos_token_id=[151645, 151643], awq=awq, attention_bias=False, name=name, fp8=fp8,
                    fp8_scheme="block128" if fp8 else "")


# Qwen3 dense checkpoints (not in the reference's registry; HF Qwen3ForCausalLM defines them): public dims, head_dim 128 free
# of hidden_size.  A local directory's config.json always overrides these.
_QWEN3_DIMS = {"0.6B": (1024, 3072, 28, 16, 8, True), "1.7B": (2048, 6144, 28, 16, 8, True),
               "4B": (2560, 9728, 36, 32, 8, True), "8B": (4096, 12288, 36, 32, 8, False),
               "14B": (5120, 17408, 40, 40, 8, False), "32B": (5120, 25600, 64, 64, 8, False)}
for _size, _d in _QWEN3_DIMS.items():
    KNOWN[f"Qwen/Qwen3-{_size}"] = _qwen3(*_d, name=f"qwen3-{_size.lower()}")
    if _size in ("4B", "8B", "14B", "32B"):
        KNOWN[f"Qwen/Qwen3-{_size}-AWQ"] = _qwen3(*_d, awq=True, name=f"qwen3-{_size.lower()}-awq")
    # FP8 e4m3 builds with 128 x 128 block scales.  Ids and dims unverified here (no hub access); a local directory's
    # config.json is the contract
    KNOWN[f"Qwen/Qwen3-{_size}-FP8"] = _qwen3(*_d, fp8=True, name=f"qwen3-{_size.lower()}-fp8")
# compressed-tensors FP8 builds of the Llama 3.x instruct models (per-channel weight scales), dims of their dense entries;
# ids unverified here as well
for _name, _dims in (("RedHatAI/Meta-Llama-3.1-8B-Instruct-FP8-dynamic", _L8), ("RedHatAI/Meta-Llama-3.1-70B-Instruct-FP8-dynamic", _L70),
                     ("RedHatAI/Llama-3.3-70B-Instruct-FP8-dynamic", _L70)):
    KNOWN[_name] = _l(**_dims, rope_scaling=LLAMA31_ROPE, fp8=True, fp8_scheme="channel",
                      name=_name.split("/")[1].lower())


def rope_inv_freq(cfg: LlamaCfg) -> tuple[torch.Tensor, float]:
    """(inv_freq [D/2] fp32, attention_scaling).  Restates HF's default and
    ``llama3`` rope initialisers, which is where the reference takes them from
    (``hf_model.model.rotary_emb.inv_freq``, umbrella/models/llama.py:48-49)."""
    D = cfg.head_dim
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))
    rs = cfg.rope_scaling
    if rs and rs.get("rope_type", rs.get("type")) == "llama3":
        factor, lo, hi = rs["factor"], rs["low_freq_factor"], rs["high_freq_factor"]
        old = rs["original_max_position_embeddings"]
        low_wl, high_wl = old / lo, old / hi
        wl = 2 * math.pi / inv
        inv_l = torch.where(wl > low_wl, inv / factor, inv)
        smooth = (old / wl - lo) / (hi - lo)
        smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
        mid = ~(wl < high_wl) & ~(wl > low_wl)
        inv = torch.where(mid, smoothed, inv_l)
    return inv, 1.0


def rope_tables(cfg: LlamaCfg, max_length: int, dtype) -> tuple[torch.Tensor, torch.Tensor]:
    """cos/sin [Lmax, D] built in fp32 then cast to the model dtype
    (umbrella/models/llama.py:50-60)."""
    inv, scale = rope_inv_freq(cfg)
    freqs = torch.outer(torch.arange(max_length, dtype=torch.float32), inv)
    emb = torch.cat((freqs, freqs), dim=-1)
    return (emb.cos() * scale).to(dtype), (emb.sin() * scale).to(dtype)
