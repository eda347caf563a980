#!/usr/bin/env python
"""FP8 (e4m3, weight-only) measurements on synthetic weights; writes profiles/fp8_bench.json and prints it as one JSON line.

    python scripts/bench_fp8.py [--no-engines]

- linears: the four 70B and the four 8B layer linears at T = 1 / 13 / 64 rows in dense 16-bit, AutoAWQ int4 and FP8 IN THE SAME
  RUN (same process, same box, warm, HIP events around 50-200 launches), each with its own plan.  The yardstick of an FP8
  linear is the unchanged dense-16 kernel of the same shape beside it: us, GB/s over the weight bytes, fraction of 8 TB/s.
- engines: 70B-FP8 target + 1B draft and Qwen3-32B-FP8 + 0.6B, static Sequoia 3x4: ms per iteration, 13-row verify
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_GBS = 8000.0


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


def _linear(fmt, N, K, il, dev, gen):
    from umbrella_amd.models import fp8_format
    from umbrella_amd.models.llama import PackedLinear
    from umbrella_amd.models.synthetic import synth_awq_tensors, synth_fp8_tensors, synth_tensor
    if fmt == "dense16":
        return PackedLinear.from_dense(synth_tensor((N, K), 0.02, torch.float16, dev, gen), interleave=il)
    if fmt == "int4":
        return PackedLinear.from_awq(*synth_awq_tensors(N, K, 128, dev, gen, 0.02), interleave=il)
    w8, sc = synth_fp8_tensors(N, K, "block128", dev, gen, 0.02)
    return PackedLinear.from_fp8(w8.view(torch.uint8), fp8_format.expand_scale(sc, N, K).to(dev), interleave=il)


def linears(rows=(1, 13, 64)):
    from umbrella_amd import _lib
    from umbrella_amd.models.llama import PackedLinear
    dev, dt = "cuda:0", torch.float16
    gen = torch.Generator(device=dev).manual_seed(0)
    shapes = {"70b": {"qkv": (10240, 8192), "o": (8192, 8192), "gate_up": (57344, 8192), "down": (8192, 28672)},
              "8b": {"qkv": (6144, 4096), "o": (4096, 4096), "gate_up": (28672, 4096), "down": (4096, 14336)}}
    res = {}
    for model, lins in shapes.items():
        for name, (N, K) in lins.items():
            il = name == "gate_up"
            entry = {"N": N, "K": K}
            for fmt in ("dense16", "int4", "fp8"):
                lin = _linear(fmt, N, K, il, dev, gen)
                nbytes = sum(PackedLinear.raw_bytes(N, K, lin.awq))
                e = {"R": lin.R, "S": lin.S, "tb": lin.tb, "weight_MB": round(nbytes / 1e6, 1)}
                for T in rows:
                    x = torch.randn(T, K, device=dev, generator=gen).to(dt)
                    if il:
                        out = torch.empty(T, N // 2, dtype=dt, device=dev)
                        args = (out, x, K, lin.w, lin.meta, T, N, K, lin.awq, 1, lin.Rtb, 2, _lib.F16)
                    else:
                        out = torch.empty(lin.S, T, N, dtype=torch.float32, device=dev)
                        args = (out, x, K, lin.w, lin.meta, T, N, K, lin.awq, lin.S, lin.Rtb, 0, _lib.F16)
                    us = 1000 * timed(lambda: _lib.call("umb_gemm", *args), reps=200 if nbytes < 2e8 else 50, warm=10)
                    e[f"T{T}"] = {"us": round(us, 2), "GBs": round(nbytes / us / 1e3, 1), "hbm_frac": round(nbytes / us / 1e3 / HBM_GBS, 3)}
                entry[fmt] = e
                del lin
                torch.cuda.empty_cache()
            for T in rows:
                entry[f"fp8_over_dense16_T{T}"] = round(entry["fp8"][f"T{T}"]["us"] / entry["dense16"][f"T{T}"]["us"], 3)
            res[f"{model}_{name}"] = entry
    return res


def _fwd(m, rows, P, vocab):
    dev = "cuda:0"
    ids = torch.randint(1000, vocab - 1000, (rows,), dtype=torch.int32, device=dev)
    pos = torch.arange(P, P + rows, dtype=torch.int32, device=dev)
    pre = torch.tensor([P], dtype=torch.int32, device=dev)
    return lambda: m.forward_explicit(ids, pos, pos, pre, head_from=0)


def engine(target_name, draft_name, steps_tokens=64):
    from umbrella_amd.models.auto_model import AutoModelLM
    from umbrella_amd.speculation.speculation_utils import IdTokenizer
    from umbrella_amd.speculation.static_speculation_engine import StaticSpeculationEngine
    dt, L = torch.float16, 2048
    target = AutoModelLM.from_pretrained(target_name, dtype=dt, max_length=L)
    draft = AutoModelLM.from_pretrained(draft_name, dtype=dt, max_length=L, cuda_graph=True)
    target.alloc()
    draft.alloc()
    with open(os.path.join(ROOT, "tests", "golden", "growmaps.json")) as f:
        gm = json.load(f)["3x4"]
    eng = StaticSpeculationEngine(draft_name, target_name, growmap=gm, dtype=dt, device="cuda:0", max_length=L, safe_buffer=32,
                                  stop_distance=8, draft_model_obj=draft, target_model_obj=target, tokenizer=IdTokenizer())
    eng.initialize()
    V = target.config.vocab_size
    prompt = torch.randint(1000, V - 1000, (64,), generator=torch.Generator().manual_seed(0)).tolist()
    eng.generate(input_ids=prompt, max_new_tokens=8)                      # warm-up: graph capture
    out = eng.generate(input_ids=prompt, max_new_tokens=steps_tokens)
    ms_iter = out["time_per_output_token"] * out["avg_accept_tokens"]
    ids = torch.tensor(prompt, dtype=torch.int32, device="cuda:0")
    target.prefill_tokens(ids, 0, want_logits=False)
    verify = timed(_fwd(target, 13, len(prompt), V), reps=10, warm=2)
    res = {"ms_per_iteration": round(ms_iter, 3), "tokens": len(out["generated_tokens"]), "accept": round(out["avg_accept_tokens"], 3),
           "verify_ms_13_rows": round(verify, 3), "target_weight_GB": round(target.weight_bytes() / 1e9, 2),
           "verify_roofline_ms_at_8TBs": round(target.weight_bytes() / 8e12 * 1e3, 3)}
    del eng, target, draft
    torch.cuda.empty_cache()
    return res


def main():
    os.environ["UMBRELLA_SYNTHETIC"] = "1"
    import __graft_entry__ as g
    from umbrella_amd.models.config import KNOWN
    g.build()
    res = {"linears_fp16_activations": linears()}
    if "--no-engines" not in sys.argv:
        t70 = next(k for k, c in KNOWN.items() if c.fp8 and c.hidden_size == 8192)
        res["engine_70b_fp8_1b_3x4_fp16"] = engine(t70, "meta-llama/Llama-3.2-1B-Instruct")
        res["engine_qwen3_32b_fp8_06b_3x4_fp16"] = engine("Qwen/Qwen3-32B-FP8", "Qwen/Qwen3-0.6B")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "fp8_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
