"""CPU restatement of HF Qwen3ForCausalLM (eager attention) for the Qwen3 tests.

Seeded tiny checkpoints (``qwen3_state``), a fp32 forward over a causal prompt (``Qwen3Ref``; ``qk_norm=False`` switches the
two head norms off -- the function a runtime without them would compute), and the single op the HIP kernel implements, with
HF's roundings to the model dtype: split-sum -> per-head RMSNorm of q and k -> rotate-half RoPE (``qk_norm_rope``).
Reproduces tests/golden/qwen3_logits.npz (written by tests/golden/make_golden_qwen3.py from HF) to 1e-4."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

# the two fixture configs, both head_dim 128: (A) Hq * D = 512 != H = 256 as the 0.6B / 4B, tied; (B) 2 q / 2 kv heads, untied head
CFGS = {
    "A": dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=4, num_attention_heads=4,
              num_key_value_heads=2, head_dim=128, tie_word_embeddings=True),
    "B": dict(vocab_size=512, hidden_size=256, intermediate_size=384, num_hidden_layers=4, num_attention_heads=2,
              num_key_value_heads=2, head_dim=128, tie_word_embeddings=False),
}
COMMON = dict(rms_norm_eps=1e-6, rope_theta=1000000.0)
SEEDS = {"A": 96, "B": 90}
EMBED_STD = 0.25          # embedding (and untied head) rows: small beside the branches, so that the layers and not the token's own
                          # (tied) row decide the next token -- at std 1 the tied model copies its input whatever attention does
FINAL_NORM = 2.0          # mean of the final norm's weight: logits of magnitude ~35
# q_norm / k_norm weights per config, (mean, std) each: away from 1 and from each other.  Their product sets how sharp attention is,
# and with it both how far the logits move when the norms are dropped and how far bf16 rounding moves them.  Rounding the WEIGHTS
# alone to bf16 (the restatement on rounded weights, no runtime involved) moves the logits by this fraction of the GPU test's bf16
# tolerance: 1.0 - 2.0 at means 2 x 1.5, 0.5 - 0.65 at 1.3 x 1.2, 0.37 (A) and 0.30 (B) at the values below -- which still leave
# the no-norm logits 1.13 (A) and 1.14 (B) times further away than tests/test_qwen3.py asks.  Activation rounding needs the rest.
O_SCALE = 3.0           # o_proj rows at three times N(0, 1 / fan_in): attention, not the token's own embedding row, decides
NORMS = {"A": ((1.6, 0.3), (0.7, 0.3)), "B": ((0.6, 0.3), (2.0, 0.3))}
Q_NORM, K_NORM = (1.3, 0.3), (1.2, 0.3)          # the two-layer full-width models of tests/test_qwen3.py


def llama_cfg(kind: str, **kw):
    """the runtime's LlamaCfg of a fixture config"""
    from umbrella_amd.models.config import LlamaCfg
    c = dict(CFGS[kind], **COMMON)
    return LlamaCfg(family="qwen3", vocab_size=c["vocab_size"], hidden_size=c["hidden_size"],
                    intermediate_size=c["intermediate_size"], num_hidden_layers=c["num_hidden_layers"],
                    num_attention_heads=c["num_attention_heads"], num_key_value_heads=c["num_key_value_heads"],
                    head_dim=c["head_dim"], rms_norm_eps=c["rms_norm_eps"], rope_theta=c["rope_theta"], rope_scaling=None,
                    max_position_embeddings=40960, tie_word_embeddings=c["tie_word_embeddings"],
                    eos_token_id=kw.pop("eos", [3, 5]), name="tiny-qwen3-" + kind, **kw)


def linear_shapes(c: dict) -> dict:
    H, I, Hq, Hkv, D = c["hidden_size"], c["intermediate_size"], c["num_attention_heads"], c["num_key_value_heads"], c["head_dim"]
    return {"self_attn.q_proj": (Hq * D, H), "self_attn.k_proj": (Hkv * D, H), "self_attn.v_proj": (Hkv * D, H),
            "self_attn.o_proj": (H, Hq * D), "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}


def qwen3_state(kind: str) -> dict:
    """fp32 HF-named state dict, numpy-seeded (stable across library versions).  Linears N(0, 1/fan_in) with o_proj three
    times that, so that attention and not the token's own embedding row decides the next token; q_norm / k_norm well away
    from 1 and from each other (NORMS)"""
    c = CFGS[kind]
    rs = np.random.RandomState(SEEDS[kind])
    H, D = c["hidden_size"], c["head_dim"]

    def nrm(*shape, s):
        return torch.from_numpy((rs.standard_normal(shape) * s).astype(np.float32))
    sd = {"model.embed_tokens.weight": nrm(c["vocab_size"], H, s=EMBED_STD)}
    for i in range(c["num_hidden_layers"]):
        p = f"model.layers.{i}."
        for n, (a, b) in linear_shapes(c).items():
            sd[p + n + ".weight"] = nrm(a, b, s=(O_SCALE if n.endswith("o_proj") else 1.0) / math.sqrt(b))
        for n in ("input_layernorm", "post_attention_layernorm"):
            sd[p + n + ".weight"] = nrm(H, s=0.2) + 1.0
        sd[p + "self_attn.q_norm.weight"] = nrm(D, s=NORMS[kind][0][1]) + NORMS[kind][0][0]
        sd[p + "self_attn.k_norm.weight"] = nrm(D, s=NORMS[kind][1][1]) + NORMS[kind][1][0]
    sd["model.norm.weight"] = nrm(H, s=0.2) + FINAL_NORM
    if not c["tie_word_embeddings"]:
        sd["lm_head.weight"] = nrm(c["vocab_size"], H, s=EMBED_STD)
    return sd


# ----------------------------------------------------------------------------- ops
def rnd(x: torch.Tensor, dtype) -> torch.Tensor:
    return x.to(dtype).float() if dtype is not None else x


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float, dtype=None) -> torch.Tensor:
    """HF Qwen3RMSNorm: weight * (x_fp32 * rsqrt(mean x_fp32^2 + eps)).to(dtype), the product in dtype too"""
    xf = x.float()
    y = rnd(xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps), dtype)
    return rnd(w.float() * y, dtype)


def butterfly_sum(v: torch.Tensor) -> torch.Tensor:
    """[..., 64] fp32 -> [...]: the 64-lane sum of the HIP kernels (wave_sum in csrc/common.h), lane l adding lane l ^ o for
    o = 32, 16, ... 1 -- the order in which umb_reduce_qkv_rope_qknorm adds a head's squares and a token's deferred sums"""
    idx = torch.arange(64, device=v.device)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def head_sumsq(x: torch.Tensor) -> torch.Tensor:
    """fp32 sum of squares over the last dim (D <= 256) in the kernel's documented order: lane l holds the pairs (d, d + D/2),
    d = l + 64 i, adds a^2 + b^2 per pair, its pairs in order, then the butterfly.  Differs from .pow(2).sum(-1) in the last bit
    only; with it the restatement's 1/rms is the kernel's, bit for bit"""
    D = x.shape[-1]
    half, NP = D // 2, (D // 2 + 63) // 64
    pad = (0, 64 * NP - half)
    a = F.pad(x[..., :half].float(), pad).reshape(*x.shape[:-1], NP, 64)
    b = F.pad(x[..., half:].float(), pad).reshape(*x.shape[:-1], NP, 64)
    s = a * a + b * b
    ss = s[..., 0, :]
    for i in range(1, NP):
        ss = ss + s[..., i, :]
    return butterfly_sum(ss)


def rms_norm_kernel_order(x: torch.Tensor, w: torch.Tensor, eps: float, dtype) -> torch.Tensor:
    """rms_norm with the sum of squares added as the kernel adds it (head_sumsq) and 1 / rms correctly rounded"""
    xf = x.float()
    v = head_sumsq(xf)[..., None] / x.shape[-1] + eps
    r = (1.0 / torch.sqrt(v.double())).float()          # the fp32 nearest to 1 / sqrt(v), as the kernel forms it
    y = rnd(xf * r, dtype)
    return rnd(w.float() * y, dtype)


def rope_tables(D: int, theta: float, n: int, dtype=None):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))
    fr = torch.outer(torch.arange(n).float(), inv)
    emb = torch.cat((fr, fr), dim=-1)
    return rnd(emb.cos(), dtype), rnd(emb.sin(), dtype)


def rope_rounded(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, dtype) -> torch.Tensor:
    """apply_rotary_pos_emb in the model dtype: x [T, heads, D], cos / sin [T, D] already in dtype; every product and the sum
    rounded, as eager torch does"""
    D = x.shape[-1]
    c, s = cos.float()[:, None].to(x.device), sin.float()[:, None].to(x.device)
    r = torch.cat((-x[..., D // 2:], x[..., :D // 2]), -1)
    return rnd(rnd(x * c, dtype) + rnd(r * s, dtype), dtype)


def qk_norm_rope(acc: torch.Tensor, Hq: int, Hkv: int, D: int, q_w, k_w, eps: float, cos, sin, dtype, bias=None):
    """The op of umb_reduce_qkv_rope_qknorm on the already summed fp32 projection acc [T, (Hq + 2 Hkv) D] (HF feature order):
    round (+ bias first), head norm on q and k, RoPE with cos / sin [T, D]; returns (q [T, Hq, D], k, v [T, Hkv, D]) fp32
    holding values of `dtype`"""
    T = acc.shape[0]
    x = rnd(acc + (bias.float() if bias is not None else 0.0), dtype).view(T, Hq + 2 * Hkv, D)
    q = rms_norm_kernel_order(x[:, :Hq], q_w, eps, dtype)
    k = rms_norm_kernel_order(x[:, Hq:Hq + Hkv], k_w, eps, dtype)
    return rope_rounded(q, cos, sin, dtype), rope_rounded(k, cos, sin, dtype), x[:, Hq + Hkv:]


def attention(q, k, v, scale):
    """causal, q [T, Hq, D], k / v [T, Hkv, D] fp32 -> [T, Hq, D]"""
    T = q.shape[0]
    g = q.shape[1] // k.shape[1]
    kk, vv = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
    s = torch.einsum("thd,chd->htc", q, kk) * scale
    vis = torch.tril(torch.ones(T, T, dtype=torch.bool, device=q.device))
    s = s.masked_fill(~vis[None], float("-inf"))
    return torch.einsum("htc,chd->thd", torch.softmax(s, dim=-1), vv)


class Qwen3Ref:
    """fp32 Qwen3ForCausalLM over one causal prompt at positions 0 .. T-1"""

    def __init__(self, kind, sd: dict | None = None, qk_norm: bool = True):
        self.c = dict(CFGS[kind], **COMMON) if isinstance(kind, str) else dict(kind)      # a fixture name or a config dict
        self.sd = sd if sd is not None else qwen3_state(kind)
        self.qk_norm = qk_norm

    def forward(self, ids) -> torch.Tensor:
        c, sd = self.c, self.sd
        dev = sd["model.embed_tokens.weight"].device
        ids = torch.as_tensor(ids).reshape(-1).to(dev)
        T = ids.shape[0]
        Hq, Hkv, D, eps = c["num_attention_heads"], c["num_key_value_heads"], c["head_dim"], c["rms_norm_eps"]
        cos, sin = (t.to(dev)[:, None] for t in rope_tables(D, c["rope_theta"], T))

        def rope(x):
            return x * cos + torch.cat((-x[..., D // 2:], x[..., :D // 2]), -1) * sin
        h = sd["model.embed_tokens.weight"][ids].float()
        for i in range(c["num_hidden_layers"]):
            p = f"model.layers.{i}."
            w = lambda n: sd[p + n + ".weight"].float()          # noqa: E731
            x = rms_norm(h, w("input_layernorm"), eps)
            q = (x @ w("self_attn.q_proj").T).view(T, Hq, D)
            k = (x @ w("self_attn.k_proj").T).view(T, Hkv, D)
            v = (x @ w("self_attn.v_proj").T).view(T, Hkv, D)
            if self.qk_norm:
                q, k = rms_norm(q, w("self_attn.q_norm"), eps), rms_norm(k, w("self_attn.k_norm"), eps)
            a = attention(rope(q), rope(k), v, D ** -0.5).reshape(T, Hq * D)
            h = h + a @ w("self_attn.o_proj").T
            x = rms_norm(h, w("post_attention_layernorm"), eps)
            h = h + (F.silu(x @ w("mlp.gate_proj").T) * (x @ w("mlp.up_proj").T)) @ w("mlp.down_proj").T
        head = sd.get("lm_head.weight", sd["model.embed_tokens.weight"]).float()
        return rms_norm(h, sd["model.norm.weight"], eps) @ head.T
