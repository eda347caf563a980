"""Qwen3 dense runtime on the HIP hot path (0.6B ... 32B; not in the reference's registry).

Arithmetic of record: HF ``Qwen3ForCausalLM``.  A Llama-shaped decoder (RMSNorm, SiLU MLP, rotate-half RoPE, GQA, no
projection bias, head_dim free of hidden_size) with one more step in attention: an RMSNorm over each head's head_dim on q and
on k, after the projection and before RoPE (``Qwen3Attention.forward``),

  q = rope(q_norm(q_proj(x).view(T, Hq, D))),  k = rope(k_norm(k_proj(x).view(T, Hkv, D))),
  q_norm(y) = w * (y_fp32 * rsqrt(mean y_fp32^2 + eps)).to(dtype)                      (``Qwen3RMSNorm.forward``)

which runs in the q/k/v split-K reduce (umb_reduce_qkv_rope_qknorm).  Everything numeric runs in libumbrella_hip.so
(umb_model_forward_qwen3 and its offload twin).

Supported: dense and AWQ checkpoints, resident, ``offload=True`` (the linears stream; every norm vector stays device resident)
and ``cuda_graph=True`` (engine-captured step graphs).  Qwen3 always runs schedule 0 (8-launch split-K layers, with the
deferred RMSNorm and FM-ordered activations where the Llama runtime takes them): ``UMB_SCHED``, ``UMB_FUSED``, ``UMB_GEMV`` and
``UMB_CHAIN`` are ignored and ``use_gemv(True)`` is a no-op -- the fused, low-latency, GEMV and persistent-chain q/k/v epilogues
give a thread four rows of a head and cannot see the head's sum of squares.  Not supported (NotImplementedError): tensor
parallelism, layer pipelining (``layer_range``), Qwen3-MoE, sliding-window layer types.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib
from .._lib import UmbQwen3, UmbQwen3Norms
from .llama import Llama


class Qwen3(Llama):
    FAMILY = "qwen3"

    def __init__(self, model_name: str, **kwargs) -> None:
        kwargs["sched"] = "split"
        super().__init__(model_name, **kwargs)
        self.sched, self.fused = "split", False

    def alloc(self, **kwargs):
        if kwargs.get("layer_range") is not None:
            raise NotImplementedError("layer pipelining is not supported for Qwen3")
        super().alloc(**kwargs)
        c, dt = self.config, self.dtype
        fetch = self._tensor_source()
        D = c.head_dim
        self.qk_norms = []
        for i in range(self.num_layers):
            p = f"model.layers.{i}.self_attn."
            # synthetic source: ones, as HF initialises Qwen3RMSNorm
            self.qk_norms.append(tuple(fetch(p + n + ".weight", (D,), "norm").to(dt).reshape(-1).contiguous()
                                       for n in ("q_norm", "k_norm")))
            assert all(t.numel() == D for t in self.qk_norms[-1]), (i, D)
        self._qnorms = (UmbQwen3Norms * self.num_layers)()
        for i, (qn, kn) in enumerate(self.qk_norms):
            self._qnorms[i].q_norm, self._qnorms[i].k_norm = qn.data_ptr(), kn.data_ptr()
        q = self._q = UmbQwen3()
        q.qk_eps = c.rms_norm_eps
        q.norms = C.cast(self._qnorms, C.POINTER(UmbQwen3Norms))
        torch.cuda.synchronize()

    def use_gemv(self, on: bool):
        """No-op: the GEMV / chain / low-latency q/k/v epilogues have no head norm; every forward takes schedule 0."""
        self.gemv = False

    def _run(self, step):
        if self._tp is not None:
            raise NotImplementedError("tensor parallelism is not supported for Qwen3")
        lib = _lib.load()
        st = _lib.stream_ptr()
        if self._off is not None:
            rc = lib.umb_model_forward_qwen3_offload(C.byref(self._m), C.byref(self._ws), C.byref(step), C.byref(self._q),
                                                     C.byref(self._off), st)
        else:
            rc = lib.umb_model_forward_qwen3(C.byref(self._m), C.byref(self._ws), C.byref(step), C.byref(self._q), st)
        _lib.check(rc, "umb_model_forward_qwen3")
