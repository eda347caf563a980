#!/usr/bin/env python
"""Gemma-2 measurements (synthetic bf16 weights; prints one JSON line).

    python scripts/bench_gemma2.py                     # everything below
    python scripts/bench_gemma2.py --attn-only sliding # only the 8 k-context attention launches of one layer kind, for
    python scripts/bench_gemma2.py --attn-only global  #   rocprofv3 --kernel-trace --stats -- python ... (both kinds
                                                       #   launch the same kernel, so each gets a run of its own)

- engine: 27B target + 2B draft, static Sequoia 3x4, ms per iteration (wall, synchronised)
- verify: one 13-row target forward at the prompt's context; draft: the 3x4 tree's draft forwards (1, 3, 3, 3 rows)
- attention at an 8 k context, 13 query rows, 27B (D 128) and 9B (D 256) heads: sliding (window 4096) vs global layer
- the two unfused pieces of the Gemma layer at 27B widths, 13 rows: GELU * up in the split-K reduce (umb_reduce_gelu_mul,
  beside the Llama reduce umb_reduce_silu_mul on the same partials) and the final soft-cap pass over [13][256000]
"""
import argparse
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


def attention(kind, D, Hq, Hkv, ctx=8192, T=13, reps=50):
    """us per umb_tree_attn_gemma2 launch at `ctx` keys (cache filled with random K / V)"""
    from umbrella_amd import _lib
    dev, dt = "cuda:0", torch.bfloat16
    Lmax = ctx + 256
    kc = torch.randn(Hkv * Lmax * D, device=dev).to(dt)
    vt = torch.randn(Hkv * D * (Lmax + 32), device=dev).to(dt)
    q = torch.randn(T, Hq, D, device=dev).to(dt)
    splits = 32
    po = torch.empty(splits * T * Hq * D, device=dev)
    pml = torch.empty(splits * T * Hq * 2, device=dev)
    cnt = torch.zeros(Hkv * ((T * Hq // Hkv + 15) // 16) + 64, dtype=torch.int32, device=dev)
    out = torch.empty(T, Hq, D, dtype=dt, device=dev)
    prefix = torch.tensor([ctx], dtype=torch.int32, device=dev)
    pos = torch.arange(ctx, ctx + T, dtype=torch.int32, device=dev)
    win = 4096 if kind == "sliding" else 0
    args = (out, q, kc, vt, po, pml, prefix, None, 0, T, T, Hq, Hkv, D, Lmax, splits, D ** -0.5, 50.0, pos, win, cnt,
            _lib.dtype_code(dt))
    return 1000 * timed(lambda: _lib.call("umb_tree_attn_gemma2", *args), reps=reps)


def unfused_pieces():
    from umbrella_amd import _lib
    from umbrella_amd.models.config import KNOWN
    from umbrella_amd.models.llama import PackedLinear
    c = KNOWN["google/gemma-2-27b-it"]
    dev, T, I, V = "cuda:0", 13, c.intermediate_size, c.vocab_size
    gu = PackedLinear(2 * I, c.hidden_size, False, None, None)            # the plan only
    S = gu.S
    part = torch.randn(S, T, 2 * I, device=dev)
    act = torch.empty(T, I, dtype=torch.bfloat16, device=dev)
    gelu = 1000 * timed(lambda: _lib.call("umb_reduce_gelu_mul", part, S, T, I, act, _lib.BF16))
    silu = 1000 * timed(lambda: _lib.call("umb_reduce_silu_mul", part, S, T, I, act, _lib.BF16))
    logits = torch.randn(T, V, device=dev)
    cap = 1000 * timed(lambda: _lib.call("umb_logit_softcap", logits, logits.numel(), 30.0))
    return {"gate_up_splits": S, "reduce_gelu_mul_us": round(gelu, 2), "reduce_silu_mul_us_same_partials": round(silu, 2),
            "partials_MB": round(part.numel() * 4 / 1e6, 2), "softcap_us_13x256000": round(cap, 2)}


def engine(steps_tokens=64):
    from umbrella_amd.models.auto_model import AutoModelLM
    from umbrella_amd.speculation.speculation_utils import IdTokenizer
    from umbrella_amd.speculation.static_speculation_engine import StaticSpeculationEngine
    os.environ["UMBRELLA_SYNTHETIC"] = "1"
    dt, L = torch.bfloat16, 2048
    target = AutoModelLM.from_pretrained("google/gemma-2-27b-it", dtype=dt, max_length=L)
    draft = AutoModelLM.from_pretrained("google/gemma-2-2b-it", dtype=dt, max_length=L, cuda_graph=True)
    target.alloc()
    draft.alloc()
    with open(os.path.join(ROOT, "tests", "golden", "growmaps.json")) as f:
        gm = json.load(f)["3x4"]
    eng = StaticSpeculationEngine("google/gemma-2-2b-it", "google/gemma-2-27b-it", growmap=gm, dtype=dt, device="cuda:0",
                                  max_length=L, safe_buffer=32, stop_distance=8, draft_model_obj=draft,
                                  target_model_obj=target, tokenizer=IdTokenizer())
    eng.initialize()
    prompt = torch.randint(1000, 200000, (128,), generator=torch.Generator().manual_seed(0)).tolist()
    eng.generate(input_ids=prompt, max_new_tokens=8)                      # warm-up: graph capture
    out = eng.generate(input_ids=prompt, max_new_tokens=steps_tokens)
    ms_iter = out["time_per_output_token"] * out["avg_accept_tokens"]
    # verify / draft forwards at the same context, eager
    dev = "cuda:0"
    P = len(prompt)

    def fwd(m, rows):
        ids = torch.randint(1000, 200000, (rows,), dtype=torch.int32, device=dev)
        pos = torch.arange(P, P + rows, dtype=torch.int32, device=dev)
        pre = torch.tensor([P], dtype=torch.int32, device=dev)
        return lambda: m.forward_explicit(ids, pos, pos, pre, head_from=0)
    target.prefill_tokens(torch.tensor(prompt, dtype=torch.int32, device=dev), 0, want_logits=False)
    draft.prefill_tokens(torch.tensor(prompt, dtype=torch.int32, device=dev), 0, want_logits=False)
    verify = timed(fwd(target, 13), reps=10, warm=2)
    d1, d3 = timed(fwd(draft, 1), reps=20, warm=3), timed(fwd(draft, 3), reps=20, warm=3)
    return {"ms_per_iteration": round(ms_iter, 3), "tokens": len(out["generated_tokens"]),
            "accept": round(out["avg_accept_tokens"], 3), "verify_ms_13_rows": round(verify, 3),
            "draft_ms_1_3_3_3_rows": round(d1 + 3 * d3, 3), "target_weight_GB": round(target.weight_bytes() / 1e9, 2),
            "verify_roofline_ms_at_8TBs": round(target.weight_bytes() / 8e12 * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attn-only", choices=("sliding", "global"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    if a.attn_only:
        for D, Hq, Hkv in ((128, 32, 16), (256, 16, 8)):
            attention(a.attn_only, D, Hq, Hkv, reps=200)
        return
    res = {"attention_8k_us": {}}
    for name, (D, Hq, Hkv) in (("27B_D128", (128, 32, 16)), ("9B_D256", (256, 16, 8))):
        s, gl = attention("sliding", D, Hq, Hkv), attention("global", D, Hq, Hkv)
        res["attention_8k_us"][name] = {"sliding": round(s, 2), "global": round(gl, 2), "ratio": round(s / gl, 3)}
    res["unfused"] = unfused_pieces()
    res["engine_27b_2b_3x4_bf16"] = engine()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
