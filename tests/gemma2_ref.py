"""CPU restatement of HF Gemma2ForCausalLM (eager attention) for the Gemma-2 tests.

Seeded tiny checkpoints (``gemma2_state``), a fp32 forward over a causal prompt (``Gemma2Ref``), and the single ops the HIP
kernels implement: masked / windowed / soft-capped attention, Gemma RMSNorm, the sandwich reduce and GELU-tanh * up, the
latter two with HF's rounding to the model dtype.  Reproduces tests/golden/gemma2_logits.npz (written by
tests/golden/make_golden_gemma2.py from HF) to 1e-4."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

# the two fixture configs: (A) head_dim 256 as the 2B / 9B, (B) head_dim 128 with query_pre_attn_scalar 144 as the 27B
CFGS = {
    "A": dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=4, num_attention_heads=4,
              num_key_value_heads=2, head_dim=256, query_pre_attn_scalar=256, sliding_window=16),
    "B": dict(vocab_size=512, hidden_size=256, intermediate_size=384, num_hidden_layers=4, num_attention_heads=4,
              num_key_value_heads=2, head_dim=128, query_pre_attn_scalar=144, sliding_window=16),
}
COMMON = dict(rms_norm_eps=1e-6, rope_theta=10000.0, attn_logit_softcapping=50.0, final_logit_softcapping=30.0)
SEEDS = {"A": 71, "B": 72}


def llama_cfg(kind: str, **kw):
    """the runtime's LlamaCfg of a fixture config"""
    from umbrella_amd.models.config import LlamaCfg
    c = dict(CFGS[kind], **COMMON)
    return LlamaCfg(family="gemma2", vocab_size=c["vocab_size"], hidden_size=c["hidden_size"],
                    intermediate_size=c["intermediate_size"], num_hidden_layers=c["num_hidden_layers"],
                    num_attention_heads=c["num_attention_heads"], num_key_value_heads=c["num_key_value_heads"],
                    head_dim=c["head_dim"], rms_norm_eps=c["rms_norm_eps"], rope_theta=c["rope_theta"], rope_scaling=None,
                    max_position_embeddings=8192, tie_word_embeddings=True, eos_token_id=kw.pop("eos", [3, 5]),
                    attn_logit_softcapping=c["attn_logit_softcapping"], final_logit_softcapping=c["final_logit_softcapping"],
                    query_pre_attn_scalar=float(c["query_pre_attn_scalar"]), sliding_window=c["sliding_window"],
                    sliding_parity=0, hidden_activation="gelu_pytorch_tanh", name="tiny-gemma2-" + kind, **kw)


def gemma2_state(kind: str) -> dict:
    """fp32 HF-named state dict, numpy-seeded (stable across library versions); tied embeddings"""
    c = CFGS[kind]
    rs = np.random.RandomState(SEEDS[kind])
    H, I, Hq, Hkv, D = c["hidden_size"], c["intermediate_size"], c["num_attention_heads"], c["num_key_value_heads"], c["head_dim"]

    def nrm(*shape, s=0.06):
        return torch.from_numpy((rs.standard_normal(shape) * s).astype(np.float32))
    # the embedding at std H^-1/2, so that sqrt(H) * e has unit RMS and the layers, not the token's own (tied) row, decide the
    # next token: at std 1 the residual stream is the input embedding and the model copies its input whatever attention does
    sd = {"model.embed_tokens.weight": nrm(c["vocab_size"], H, s=H ** -0.5)}
    shapes = {"self_attn.q_proj": (Hq * D, H), "self_attn.k_proj": (Hkv * D, H), "self_attn.v_proj": (Hkv * D, H),
              "self_attn.o_proj": (H, Hq * D), "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}
    for i in range(c["num_hidden_layers"]):
        p = f"model.layers.{i}."
        for n, (a, b) in shapes.items():
            sd[p + n + ".weight"] = nrm(a, b, s=1.0 / math.sqrt(b))
        for n in ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm"):
            sd[p + n + ".weight"] = nrm(H, s=0.2) + (2.0 if n.startswith("post") else 0.0)   # branches 3x the embedding
    sd["model.norm.weight"] = nrm(H, s=0.2) + 3.0                                            # logits of O(5): clear margins
    return sd


# ----------------------------------------------------------------------------- ops
def rnd(x: torch.Tensor, dtype) -> torch.Tensor:
    return x.to(dtype).float() if dtype is not None else x


def gemma_norm(x: torch.Tensor, w: torch.Tensor, eps: float, dtype=None) -> torch.Tensor:
    """HF Gemma2RMSNorm: fp32 x * rsqrt(mean x^2 + eps) * (1 + w), rounded once to dtype"""
    xf = x.float()
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return rnd(y * (1.0 + w.float()), dtype)


def sandwich(partial_sum: torch.Tensor, h: torch.Tensor, w_post, w_next, eps, dtype):
    """(h, xn) after o / down: y = round(proj), h = round(h + round(norm(y))), xn = norm(h) with the next weight"""
    y = rnd(partial_sum, dtype)
    hh = rnd(h.float() + gemma_norm(y, w_post, eps, dtype), dtype)
    return hh, (gemma_norm(hh, w_next, eps, dtype) if w_next is not None else None)


def gelu_mul(gate: torch.Tensor, up: torch.Tensor, dtype):
    """Gemma2MLP act_fn(gate) * up, gate / up / gelu / product each in the model dtype"""
    g, u = rnd(gate, dtype), rnd(up, dtype)
    return rnd(rnd(F.gelu(g, approximate="tanh"), dtype) * u, dtype)


def attention(q, k, v, scale, softcap, visible):
    """q [T, Hq, D], k / v [C, Hkv, D] fp32; visible bool [T, C] -> [T, Hq, D] (eager_attention_forward, fp32)"""
    T, Hq, D = q.shape
    g = Hq // k.shape[1]
    kk, vv = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
    s = torch.einsum("thd,chd->htc", q.float(), kk.float()) * scale
    if softcap:
        s = torch.tanh(s / softcap) * softcap
    s = s.masked_fill(~visible[None], float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("htc,chd->thd", p, vv.float())


def window_mask(qpos: torch.Tensor, C: int, window: int, base: torch.Tensor | None = None):
    """causal-by-position (key slot == position) visibility, limited to p - c < window when window > 0"""
    c = torch.arange(C, device=qpos.device)[None]
    vis = c <= qpos[:, None] if base is None else base.clone()
    if window:
        vis &= (qpos[:, None] - c) < window
    return vis


def rope(x, pos, theta):
    D = x.shape[-1]
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.int64, device=x.device).float() / D))
    fr = torch.outer(pos.float(), inv)
    emb = torch.cat((fr, fr), dim=-1)
    cos, sin = emb.cos()[:, None], emb.sin()[:, None]
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    return x * cos + torch.cat((-x2, x1), dim=-1) * sin


class Gemma2Ref:
    """fp32 Gemma2ForCausalLM over one causal prompt at positions 0 .. T-1"""

    def __init__(self, kind, sd: dict | None = None):
        self.c = dict(CFGS[kind], **COMMON) if isinstance(kind, str) else dict(kind)      # a fixture name or a config dict
        self.sd = sd if sd is not None else gemma2_state(kind)

    def forward(self, ids) -> torch.Tensor:
        c, sd = self.c, self.sd
        dev = sd["model.embed_tokens.weight"].device
        ids = torch.as_tensor(ids).reshape(-1).to(dev)
        T = ids.shape[0]
        H, Hq, Hkv, D, eps = c["hidden_size"], c["num_attention_heads"], c["num_key_value_heads"], c["head_dim"], c["rms_norm_eps"]
        pos = torch.arange(T, device=dev)
        h = sd["model.embed_tokens.weight"][ids].float() * torch.tensor(H ** 0.5)
        scale = c["query_pre_attn_scalar"] ** -0.5
        for i in range(c["num_hidden_layers"]):
            p = f"model.layers.{i}."
            w = lambda n: sd[p + n + ".weight"].float()          # noqa: E731
            x = gemma_norm(h, w("input_layernorm"), eps)
            q = rope((x @ w("self_attn.q_proj").T).view(T, Hq, D), pos, c["rope_theta"])
            k = rope((x @ w("self_attn.k_proj").T).view(T, Hkv, D), pos, c["rope_theta"])
            v = (x @ w("self_attn.v_proj").T).view(T, Hkv, D)
            vis = window_mask(pos, T, c["sliding_window"] if i % 2 == 0 else 0)
            a = attention(q, k, v, scale, c["attn_logit_softcapping"], vis).reshape(T, Hq * D)
            h = h + gemma_norm(a @ w("self_attn.o_proj").T, w("post_attention_layernorm"), eps)
            x = gemma_norm(h, w("pre_feedforward_layernorm"), eps)
            m = F.gelu(x @ w("mlp.gate_proj").T, approximate="tanh") * (x @ w("mlp.up_proj").T)
            h = h + gemma_norm(m @ w("mlp.down_proj").T, w("post_feedforward_layernorm"), eps)
        z = gemma_norm(h, sd["model.norm.weight"], eps) @ sd["model.embed_tokens.weight"].float().T
        cap = c["final_logit_softcapping"]
        return torch.tanh(z / cap) * cap
