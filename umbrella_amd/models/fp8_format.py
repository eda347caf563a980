"""FP8 (OCP ``float8_e4m3fn``) weight-only checkpoints: config parsing, scale shapes, checks.  Host code, no GPU.

Two published forms are read (both store ``<linear>.weight`` as float8_e4m3fn):

  "block128"  ``quant_method == "fp8"`` with ``weight_block_size == [128, 128]`` (the Qwen/Qwen3-*-FP8 builds):
              ``<linear>.weight_scale_inv`` fp32 [ceil(N/128)][K/128], W = e4m3(weight) * scale of the block
  "tensor" /  ``quant_method == "compressed-tensors"`` whose weight scheme is 8-bit ``float``, symmetric, strategy
  "channel"   ``tensor`` or ``channel``: ``<linear>.weight_scale`` of shape [1], scalar or [N, 1]

The kernels take ONE scale shape, fp32 [N][K/128] (umb_fp8_repack): ``expand_scale`` produces it.  The runtime is weight-only
(W8A16): activation-quantization settings of the checkpoint (dynamic / static input scales) are ignored.
"""
from __future__ import annotations

import torch

GROUP = 128
SCALE_SUFFIX = {"block128": ".weight_scale_inv", "tensor": ".weight_scale", "channel": ".weight_scale"}


def parse_quant_config(q: dict | None):
    """``quantization_config`` of a config.json -> None (not FP8) or "block128" / "tensor" / "channel".  Raises ValueError
    naming the offending key for FP8 forms this runtime does not compute."""
    if not q:
        return None
    method = q.get("quant_method")
    if method == "fp8":
        fmt = str(q.get("fmt", "e4m3")).lower()
        if "e5m2" in fmt or "fnuz" in fmt or fmt not in ("e4m3", "float8_e4m3fn", "e4m3fn"):
            raise ValueError(f"quantization_config.fmt = {q.get('fmt')!r}: only OCP e4m3 (float8_e4m3fn) weights are supported")
        wbs = q.get("weight_block_size")
        if wbs is None or list(wbs) != [GROUP, GROUP]:
            raise ValueError(f"quantization_config.weight_block_size = {wbs!r}: only [128, 128] block scales are supported")
        return "block128"
    if method == "compressed-tensors":
        groups = q.get("config_groups") or {}
        scheme = None
        for gname, g in groups.items():
            w = (g or {}).get("weights") or {}
            key = f"quantization_config.config_groups.{gname}.weights"
            if w.get("type") != "float":
                return None             # int8 / W4A16 ... compressed-tensors builds: not FP8, read as they were before FP8 existed
            if int(w.get("num_bits", 0)) != 8:
                raise ValueError(f"{key}.num_bits = {w.get('num_bits')!r}: only 8-bit float (e4m3) weights are supported")
            if not w.get("symmetric", True):
                raise ValueError(f"{key}.symmetric = {w.get('symmetric')!r}: only symmetric FP8 weights are supported")
            strat = w.get("strategy")
            if strat not in ("tensor", "channel"):
                raise ValueError(f"{key}.strategy = {strat!r}: only 'tensor' and 'channel' scales are supported")
            if scheme is not None and scheme != strat:
                raise ValueError(f"{key}.strategy = {strat!r}: config groups with different weight strategies")
            scheme = strat
        return scheme                   # None: no weight scheme at all -- not FP8
    return None


def check_weight(name: str, w8: torch.Tensor) -> torch.Tensor:
    """A projection weight of an FP8 checkpoint -> its uint8 code view; ValueError naming ``name`` for e5m2 / fnuz dtypes,
    non-FP8 tensors and NaN codes ((b & 0x7f) == 0x7f: OCP e4m3fn has no infinities, both are NaN)."""
    dt = w8.dtype
    if dt != torch.float8_e4m3fn:
        what = "e5m2 weights" if dt == getattr(torch, "float8_e5m2", None) else \
            "fnuz dtypes" if "fnuz" in str(dt) else "this dtype"
        raise ValueError(f"{name}: dtype {dt} ({what}) is not supported; FP8 checkpoints must store OCP float8_e4m3fn")
    codes = w8.contiguous().view(torch.uint8)
    if bool(((codes & 0x7F) == 0x7F).any()):
        raise ValueError(f"{name}: the FP8 weight holds NaN codes ((b & 0x7f) == 0x7f)")
    return codes


def check_head(keys, dtype_of) -> None:
    """An FP8 lm_head is refused (the head stays 16-bit).  keys: tensor names; dtype_of(name) -> a torch dtype or the
    safetensors dtype string ("F8_E4M3", "F8_E5M2")."""
    for k in ("lm_head.weight_scale", "lm_head.weight_scale_inv"):
        if k in keys:
            raise ValueError(f"{k}: an FP8 lm_head is not supported (the head must be a 16-bit tensor)")
    if "lm_head.weight" in keys and ("float8" in str(dtype_of("lm_head.weight")) or str(dtype_of("lm_head.weight")).upper().startswith("F8")):
        raise ValueError("lm_head.weight: an FP8 lm_head is not supported (the head must be a 16-bit tensor)")


def expand_scale(scale: torch.Tensor, N: int, K: int, name: str = "weight_scale") -> torch.Tensor:
    """Per-tensor ([1] or scalar), per-channel ([N, 1] / [N]) or 128 x 128 block ([ceil(N/128)][K/128]) scale ->
    fp32 [N][K/128], the one shape umb_fp8_repack reads."""
    assert K % GROUP == 0, (name, K)
    KG = K // GROUP
    s = scale.detach().to(torch.float32)
    if s.numel() == 1:
        return s.reshape(1, 1).expand(N, KG).contiguous()
    if s.numel() == N and (s.dim() == 1 or (s.dim() == 2 and s.shape[1] == 1)):
        return s.reshape(N, 1).expand(N, KG).contiguous()
    if s.dim() == 2 and tuple(s.shape) == ((N + GROUP - 1) // GROUP, KG):
        return s.repeat_interleave(GROUP, dim=0)[:N].contiguous()
    raise ValueError(f"{name}: scale shape {tuple(scale.shape)} fits neither per-tensor, per-channel [{N}, 1] nor "
                     f"128 x 128 blocks [{(N + GROUP - 1) // GROUP}, {KG}] of a [{N}, {K}] weight")


def stack(parts):
    """[(codes uint8 [N_i][K], scale_rows fp32 [N_i][K/128]), ...] -> the fused linear's (codes, scale_rows): q|k|v and
    gate|up are concatenated along N, each part keeping its own scales."""
    return (torch.cat([p[0] for p in parts], dim=0).contiguous(), torch.cat([p[1] for p in parts], dim=0).contiguous())


def dequant(codes: torch.Tensor, scale_rows: torch.Tensor) -> torch.Tensor:
    """fp32 W = e4m3(codes) * scale (rounded once to fp32): what a dense oracle model is given."""
    N, K = codes.shape
    w = codes.view(torch.float8_e4m3fn).to(torch.float32)
    return (w.view(N, K // GROUP, GROUP) * scale_rows.to(w.device).view(N, K // GROUP, 1)).view(N, K)


def quantize(w: torch.Tensor, scheme: str):
    """Round-to-nearest FP8 quantisation of a dense [N, K] weight (tests / synthetic fixtures): (float8_e4m3fn weight,
    scale tensor in the checkpoint shape of ``scheme``)."""
    w = w.detach().to(torch.float32)
    N, K = w.shape
    if scheme == "tensor":
        s = (w.abs().max().clamp_min(1e-12) / 448.0).reshape(1)
        full = s.expand(N, K)
    elif scheme == "channel":
        s = (w.abs().amax(dim=1, keepdim=True).clamp_min(1e-12) / 448.0)
        full = s.expand(N, K)
    elif scheme == "block128":
        nb = (N + GROUP - 1) // GROUP
        pad = torch.zeros(nb * GROUP, K, dtype=torch.float32)
        pad[:N] = w
        s = (pad.view(nb, GROUP, K // GROUP, GROUP).abs().amax(dim=(1, 3)).clamp_min(1e-12) / 448.0)
        full = s.repeat_interleave(GROUP, 0).repeat_interleave(GROUP, 1)[:N]
    else:
        raise ValueError(scheme)
    q = (w / full).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q, s.to(torch.float32).contiguous()
