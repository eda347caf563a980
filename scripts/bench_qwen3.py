#!/usr/bin/env python
"""Qwen3 measurements (synthetic fp16 weights; prints one JSON line).

    python scripts/bench_qwen3.py

- engine: 32B-AWQ target + 0.6B draft, static Sequoia 3x4, ms per iteration (wall, synchronised); verify: one 13-row
  target forward at the prompt's context; draft: the 3x4 tree's draft forwards (1, 3, 3, 3 rows)
- the q/k/v reduce with the head norm (umb_reduce_qkv_rope_qknorm) beside umb_reduce_qkv_rope2 on the same partials, at the
  32B and 0.6B q/k/v shapes and 1 / 3 / 13 / 257 rows: the cost of the head norm per layer
- the 0.6B and 1.7B draft forward at 1 and 3 rows on schedule 0 (what Qwen3 runs) beside a family="llama" config of the
  same dims on its default draft path (GEMV kernels / persistent chain).  The second computes the WRONG function for Qwen3
  (no head norms); its time is what a fused Qwen3 draft path could approach
"""
import dataclasses
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def reduce_cost(name, rows=(1, 3, 13, 257)):
    """us per launch: {rows: {"qknorm": .., "plain": .., "delta": ..}} at `name`'s q/k/v shape and split plan"""
    from umbrella_amd import _lib
    from umbrella_amd.models.config import KNOWN
    from umbrella_amd.models.llama import PackedLinear
    c = KNOWN[name]
    dev, dt = "cuda:0", torch.float16
    Hq, Hkv, D, Lmax = c.num_attention_heads, c.num_key_value_heads, c.head_dim, 2048
    N = (Hq + 2 * Hkv) * D
    plan = PackedLinear(N, c.hidden_size, c.awq, None, None)               # the plan only
    lib = _lib.load()
    cos = torch.randn(Lmax, D, device=dev).to(dt)
    sin = torch.randn(Lmax, D, device=dev).to(dt)
    qw, kw = torch.ones(D, dtype=dt, device=dev), torch.ones(D, dtype=dt, device=dev)
    kc = torch.zeros(Hkv * Lmax * D, dtype=dt, device=dev)
    vt = torch.zeros(Hkv * D * (Lmax + 32), dtype=dt, device=dev)
    out = {"N": N, "S_plan": plan.S}
    for T in rows:
        S = lib.umb_gemm_wide_split(T, N, plan.S)
        part = torch.randn(S, T, N, device=dev)
        pos = torch.arange(100, 100 + T, dtype=torch.int32, device=dev)
        q = torch.empty(T, Hq, D, dtype=dt, device=dev)
        base = (part, S, T, Hq, Hkv, D, Lmax, pos, pos, cos, sin, q, kc, vt, 1, None, None, 0, 0, 0.0, 0.0)
        a = 1000 * timed(lambda: _lib.call("umb_reduce_qkv_rope_qknorm", *base, qw, kw, 1e-6, _lib.F16), reps=200, warm=20)
        b = 1000 * timed(lambda: _lib.call("umb_reduce_qkv_rope2", *base, _lib.F16), reps=200, warm=20)
        out[str(T)] = {"S": S, "qknorm_us": round(a, 2), "plain_us": round(b, 2), "delta_us": round(a - b, 2)}
    return out


def _fwd(m, rows, P, vocab):
    dev = "cuda:0"
    ids = torch.randint(1000, vocab - 1000, (rows,), dtype=torch.int32, device=dev)
    pos = torch.arange(P, P + rows, dtype=torch.int32, device=dev)
    pre = torch.tensor([P], dtype=torch.int32, device=dev)
    return lambda: m.forward_explicit(ids, pos, pos, pre, head_from=0)


def draft_paths(name, P=128):
    """ms per forward at 1 / 3 rows: Qwen3 on schedule 0 vs the same dims as a Llama-family draft (GEMV / chain)"""
    from umbrella_amd.models.config import KNOWN
    from umbrella_amd.models.llama import Llama
    from umbrella_amd.models.qwen3 import Qwen3
    dt, dev = torch.float16, "cuda:0"
    cfg = KNOWN[name]
    prompt = torch.randint(1000, 150000, (P,), dtype=torch.int32, device=dev)
    res = {}
    for label, klass, c in (("qwen3_schedule0", Qwen3, cfg),
                            ("llama_family_draft_path_wrong_function", Llama, dataclasses.replace(cfg, family="llama"))):
        m = klass(name, max_length=2048, device=dev, dtype=dt, config=c, cuda_graph=True)
        m.alloc()
        m.use_gemv(True)
        m.prefill_tokens(prompt, 0, want_logits=False)
        res[label] = {"ms_1_row": round(timed(_fwd(m, 1, P, cfg.vocab_size), reps=50, warm=5), 4),
                      "ms_3_rows": round(timed(_fwd(m, 3, P, cfg.vocab_size), reps=50, warm=5), 4),
                      "gemv": bool(m.gemv), "chain": bool(getattr(m, "chain", False))}
        del m
        torch.cuda.empty_cache()
    return res


def engine(steps_tokens=64):
    from umbrella_amd.models.auto_model import AutoModelLM
    from umbrella_amd.speculation.speculation_utils import IdTokenizer
    from umbrella_amd.speculation.static_speculation_engine import StaticSpeculationEngine
    dt, L = torch.float16, 2048
    target = AutoModelLM.from_pretrained("Qwen/Qwen3-32B-AWQ", dtype=dt, max_length=L)
    draft = AutoModelLM.from_pretrained("Qwen/Qwen3-0.6B", dtype=dt, max_length=L, cuda_graph=True)
    target.alloc()
    draft.alloc()
    with open(os.path.join(ROOT, "tests", "golden", "growmaps.json")) as f:
        gm = json.load(f)["3x4"]
    eng = StaticSpeculationEngine("Qwen/Qwen3-0.6B", "Qwen/Qwen3-32B-AWQ", growmap=gm, dtype=dt, device="cuda:0",
                                  max_length=L, safe_buffer=32, stop_distance=8, draft_model_obj=draft,
                                  target_model_obj=target, tokenizer=IdTokenizer())
    eng.initialize()
    # a 64-token prompt: one prefill chunk of 64 rows, outside the wide-GEMM row counts of DESIGN.md's empty-split list
    prompt = torch.randint(1000, 150000, (64,), generator=torch.Generator().manual_seed(0)).tolist()
    eng.generate(input_ids=prompt, max_new_tokens=8)                      # warm-up: graph capture
    out = eng.generate(input_ids=prompt, max_new_tokens=steps_tokens)
    ms_iter = out["time_per_output_token"] * out["avg_accept_tokens"]
    P, V = len(prompt), target.config.vocab_size
    ids = torch.tensor(prompt, dtype=torch.int32, device="cuda:0")
    target.prefill_tokens(ids, 0, want_logits=False)
    draft.prefill_tokens(ids, 0, want_logits=False)
    verify = timed(_fwd(target, 13, P, V), reps=10, warm=2)
    d1, d3 = timed(_fwd(draft, 1, P, V), reps=20, warm=3), timed(_fwd(draft, 3, P, V), reps=20, warm=3)
    return {"ms_per_iteration": round(ms_iter, 3), "tokens": len(out["generated_tokens"]),
            "accept": round(out["avg_accept_tokens"], 3), "verify_ms_13_rows": round(verify, 3),
            "draft_ms_1_3_3_3_rows": round(d1 + 3 * d3, 3), "target_weight_GB": round(target.weight_bytes() / 1e9, 2),
            "verify_roofline_ms_at_8TBs": round(target.weight_bytes() / 8e12 * 1e3, 3)}


def main():
    os.environ["UMBRELLA_SYNTHETIC"] = "1"
    import __graft_entry__ as g
    g.build()
    res = {"reduce_us": {n: reduce_cost(n) for n in ("Qwen/Qwen3-32B-AWQ", "Qwen/Qwen3-0.6B")},
           "draft_forward_ms": {n: draft_paths(n) for n in ("Qwen/Qwen3-0.6B", "Qwen/Qwen3-1.7B")}}
    res["engine_32b_awq_06b_3x4_fp16"] = engine()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
