"""Gemma-2 runtime on the HIP hot path (the reference's Gemma2, umbrella/models/gemma.py + gemma_layer.py).

Arithmetic of record: HF ``Gemma2ForCausalLM`` (eager attention).  Per decoder layer

  xn = gemma_norm(h, input_layernorm)            gemma_norm(x, w) = x * rsqrt(mean x^2 + eps) * (1 + w), fp32, one rounding
  q, k, v = qkv(xn) (+ RoPE);  attention with scores cap * tanh(q.k * query_pre_attn_scalar^-1/2 / cap) and, on the sliding
            layers (the even ones), keys more than sliding_window - 1 positions back hidden
  h = h + gemma_norm(o_proj(attn), post_attention_layernorm)
  h = h + gemma_norm(down(gelu_tanh(gate(x)) * up(x)), post_feedforward_layernorm),  x = gemma_norm(h, pre_feedforward_layernorm)

with the embedding scaled by round(sqrt(H)) and the logits soft-capped, 30 * tanh(z / 30), in fp32 after the lm_head's
16-bit rounding.  Everything numeric runs in libumbrella_hip.so (umb_model_forward_gemma2 and its offload twin).

Supported: resident, ``offload=True`` (the linears stream; the four norm vectors stay device resident) and
``cuda_graph=True`` (engine-captured step graphs).  Gemma always runs schedule 0 (8-launch split-K layers, here 9 launches)
with row-major activations: ``UMB_SCHED`` and ``UMB_FUSED`` are ignored, ``use_gemv(True)`` is a no-op.  Not supported
(NotImplementedError): AWQ checkpoints, tensor parallelism, layer pipelining (``layer_range``).
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib
from .._lib import UmbGemma2, UmbGemma2Norms
from .llama import Llama


class Gemma2(Llama):
    FAMILY = "gemma2"
    INTERLEAVE_GU = False     # gate/up as a plain [gate; up] stack: GELU * up runs in the split-K reduce (umb_reduce_gelu_mul)

    def __init__(self, model_name: str, **kwargs) -> None:
        kwargs["sched"] = "split"
        super().__init__(model_name, **kwargs)
        c = self.config
        if c.awq:
            raise NotImplementedError("AWQ Gemma-2 checkpoints are not supported")
        if c.fp8:
            raise NotImplementedError("FP8 Gemma-2 checkpoints are not supported")
        if c.hidden_activation not in ("gelu_pytorch_tanh", "gelu_tanh"):
            raise NotImplementedError(f"Gemma-2 MLP activation {c.hidden_activation!r} (only gelu_pytorch_tanh)")
        self.sched, self.fused = "split", False

    def _tensor_source(self):
        fetch = super()._tensor_source()
        if getattr(fetch, "gen", None) is None:
            return fetch

        def synth(name, shape, kind):             # HF initialises Gemma norm weights to 0 (the scale is 1 + w)
            if kind == "norm":
                return torch.zeros(shape, dtype=self.dtype, device=self.device)
            return fetch(name, shape, kind)
        synth.gen, synth.resid_scale = fetch.gen, fetch.resid_scale
        return synth

    def alloc(self, **kwargs):
        if kwargs.get("layer_range") is not None:
            raise NotImplementedError("layer pipelining is not supported for Gemma-2")
        super().alloc(**kwargs)
        c, dt = self.config, self.dtype
        fetch = self._tensor_source()
        H = c.hidden_size
        self.ff_norms = []
        for i in range(self.num_layers):
            p = f"model.layers.{i}."
            self.ff_norms.append(tuple(fetch(p + n + ".weight", (H,), "norm").to(dt).contiguous()
                                       for n in ("pre_feedforward_layernorm", "post_feedforward_layernorm")))
        self._gnorms = (UmbGemma2Norms * self.num_layers)()
        for i, (pre, post) in enumerate(self.ff_norms):
            self._gnorms[i].pre_ff, self._gnorms[i].post_ff = pre.data_ptr(), post.data_ptr()
        g = self._g = UmbGemma2()
        g.attn_softcap, g.final_softcap = c.attn_logit_softcapping, c.final_logit_softcapping
        g.embed_scale = float(torch.tensor(H ** 0.5, dtype=dt))         # HF: the normalizer is a tensor of the model dtype
        g.window, g.slide_parity = c.sliding_window, c.sliding_parity
        g.norms = C.cast(self._gnorms, C.POINTER(UmbGemma2Norms))
        self._m.attn_scale = c.attn_scale
        torch.cuda.synchronize()

    def use_gemv(self, on: bool):
        """No-op: Gemma-2 has no GEMV / chain / low-latency kernels; every forward takes schedule 0."""
        self.gemv = False

    def _run(self, step):
        if self._tp is not None:
            raise NotImplementedError("tensor parallelism is not supported for Gemma-2")
        lib = _lib.load()
        st = _lib.stream_ptr()
        if self._off is not None:
            rc = lib.umb_model_forward_gemma2_offload(C.byref(self._m), C.byref(self._ws), C.byref(step), C.byref(self._g),
                                                      C.byref(self._off), st)
        else:
            rc = lib.umb_model_forward_gemma2(C.byref(self._m), C.byref(self._ws), C.byref(step), C.byref(self._g), st)
        _lib.check(rc, "umb_model_forward_gemma2")
