#!/usr/bin/env python
"""Headline benchmark: tokens/s at batch 1, speculative decoding on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]

--dump-outputs DIR writes what the last timed step computed (emitted token ids, the target's verify logits) as .npy
files, so that two builds can be compared output for output on identical seeded inputs.

A "step" is one speculative iteration of the hot path (draft-tree expand + target verify +
accept scan + KV compaction) on synthetic input.  Default workload = the configuration
BASELINE.json's metric is quoted on that fits one GPU: Llama-3.1-70B-Instruct-AWQ-INT4 target +
Llama-3.2-1B draft, static Sequoia 3x4 tree (T = 13), greedy, max_length 2048 -- the reference's
configs/greedy_config_48gb.json pairing -- with random-init weights of the exact shapes
(no checkpoints offline) and a random 128-token prompt already resident in HBM.

Random draft/target pairs accept ~0 drafted tokens, so acceptance is an INPUT here: the
controllable-acceptance draft (StaticSpeculationEngine.set_oracle_draft) places the target's
own greedy token at the rank-r child with probability acc[r] (default: the reference's
DEFAULT_ACC vector, umbrella/sequoia_utils.py:7).  Every draft / verify kernel still runs;
`accept_len` is reported next to the value, and `value_raw_draft` is the same loop with the
knob off (accept ~1.0).

N = 1 also reports, on the same JSON line: `roofline` (live HIP-event timing of the dominant kernel), `secondary`
(BASELINE configs 2-4, bounded step counts, each with the rate that bounds it) and `cpu_baseline` (the oracle on the
host cores).

N > 1: one rank per GPU.  Launched by `python -m torch.distributed.run ... bench.py --gpus N ...` the ranks come from
the environment; launched as plain `python bench.py --gpus N` the script starts itself again, as a child process,
under torch.distributed.run with N ranks (and refuses to run if the box has fewer than N GPUs).  The headline `value` at
N > 1 is N independent requests, one engine replica per GPU, no data-path collective ("scaling": "weak"; a batch-1
request is a sequential chain of layers and does not shard for speed); the timed region is bracketed by barriers and
the max over ranks is used.  The same line then carries `pp` (the target's layers sharded over the N ranks, RCCL
send/recv of the [T, H] activation -- BASELINE config 5) and `tp` (every layer split over the N ranks, two
all-reduces per layer), each ONE request over all N GPUs measured after the replicas.  A watchdog ends a phase that
hangs and still prints the line.
"""
from __future__ import annotations

import argparse
import json
import os

os.environ.setdefault("UMBRELLA_SYNTHETIC", "1")   # benchmarks run on seeded random weights of the exact shapes (no checkpoints offline)
import sys
import threading
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "70b-awq+1b": dict(target="hugging-quants/Meta-Llama-3.1-70B-Instruct-AWQ-INT4",
                       draft="meta-llama/Llama-3.2-1B-Instruct", dtype="fp16", tree="3x4",
                       desc="Llama-3.1-70B-Instruct-AWQ-INT4 target + Llama-3.2-1B draft, static Sequoia 3x4 (T=13), greedy, "
                            "on-device (configs/greedy_config_48gb.json pairing)"),
    "8b+1b": dict(target="meta-llama/Llama-3.1-8B-Instruct", draft="meta-llama/Llama-3.2-1B-Instruct", dtype="bf16",
                  tree="5x6", desc="Llama-3.1-8B-Instruct target + Llama-3.2-1B draft, bf16, static Sequoia 5x6 (T=31), greedy"),
    "1b+1b": dict(target="meta-llama/Llama-3.2-1B-Instruct", draft="meta-llama/Llama-3.2-1B-Instruct", dtype="fp16",
                  tree="3x4", desc="Llama-3.2-1B target + Llama-3.2-1B draft, fp16, static Sequoia 3x4, greedy"),
    # plumbing check of the multi-rank paths on small boxes / in tests: NOT a benchmark configuration
    "tiny": dict(target="umb-test/tiny-target", draft="umb-test/tiny-draft", dtype="fp16", tree="3x4", vocab_hi=500,
                 desc="tiny seeded Llama pair (tests only)"),
}
ACC_5x6 = [0.5, 0.2, 0.12, 0.08, 0.05, 0.03]
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling
MFMA_PEAK_TFLOPS = 2500.0      # dense fp16 / bf16 MFMA peak (MI355X_MICROARCH.md)
T70 = "hugging-quants/Meta-Llama-3.1-70B-Instruct-AWQ-INT4"
D1B = "meta-llama/Llama-3.2-1B-Instruct"
D8BAWQ = "hugging-quants/Meta-Llama-3.1-8B-Instruct-AWQ-INT4"


def register_tiny():
    """the `tiny` workload's two architectures (the golden fixtures' shapes), registered like hub ids"""
    from umbrella_amd.models.auto_model import AutoModelLM
    from umbrella_amd.models.config import KNOWN, LLAMA3_ROPE, LlamaCfg
    from umbrella_amd.models.llama import Llama
    tiny = {"umb-test/tiny-target": LlamaCfg(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=4,
                                             num_attention_heads=4, num_key_value_heads=2, head_dim=64, rope_scaling=LLAMA3_ROPE,
                                             eos_token_id=[3, 5], name="tiny-target"),
            "umb-test/tiny-draft": LlamaCfg(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                                            num_attention_heads=2, num_key_value_heads=1, head_dim=64, rope_scaling=LLAMA3_ROPE,
                                            tie_word_embeddings=True, eos_token_id=[3, 5], name="tiny-draft")}
    for k, v in tiny.items():
        KNOWN[k] = v
        for table in (AutoModelLM._MODEL_MAPPING, AutoModelLM._OFFLOAD_MODEL_MAPPING, AutoModelLM._CUDAGRAPH_MODEL_MAPPING):
            table[k] = Llama


# ------------------------------------------------------------------ launch plumbing
def dist_env():
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    return rank, world, local


def share_gpu() -> bool:
    """tests on a one-GPU box: every rank drives cuda:0 and the ranks talk over gloo (host staged)"""
    on = os.environ.get("UMB_BENCH_SHARE_GPU", "0") == "1"
    if on:
        os.environ["UMB_CHAIN"] = "0"        # the persistent chain needs the device to itself (csrc/chain.hip)
    return on


def self_launch(args):
    """`python bench.py --gpus N` (N > 1) outside torch.distributed.run: start the N ranks ourselves."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    import signal
    import subprocess
    if not (args.dry_run or share_gpu()):
        # counted in a child process: the launcher starts the ranks and never opens the GPU itself
        probe = "import torch; print(torch.cuda.device_count() if torch.cuda.is_available() else 0)"
        have = int(subprocess.run([sys.executable, "-c", probe], capture_output=True, text=True, check=True).stdout.split()[-1])
        if have < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: this box has {have} GPU(s); refusing to report an "
                             f"{args.gpus}-GPU number from fewer devices")
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    sys.stdout.flush()
    child = subprocess.Popen(cmd)
    signal.signal(signal.SIGTERM, lambda *_: child.terminate())
    rc = child.wait()
    raise SystemExit(rc if rc >= 0 else 128 - rc)     # killed by signal n: exit 128 + n, as a shell reports it


class Watchdog:
    """A phase that never returns (a rank died, a collective hangs) must not take the bench line with it: after the
    deadline rank 0 prints the line with what it has and every rank leaves."""

    def __init__(self, rank, emit):
        self.rank, self.emit = rank, emit
        self.deadline, self.phase = None, None
        self.lock = threading.Lock()
        threading.Thread(target=self._run, daemon=True).start()

    def arm(self, phase, seconds):
        with self.lock:
            self.phase, self.deadline = phase, time.time() + seconds

    def disarm(self):
        with self.lock:
            self.deadline = None

    def _run(self):
        while True:
            time.sleep(0.5)
            with self.lock:
                late = self.deadline is not None and time.time() > self.deadline
                phase = self.phase
            if late:
                try:
                    if self.rank == 0:
                        self.emit(f"timeout in phase '{phase}'")
                    else:
                        time.sleep(3.0)         # rank 0 prints first: a worker that exits makes the launcher stop the others
                finally:
                    sys.stdout.flush()
                    os._exit(3)                 # the line is out ("status": "sharded phase failed: timeout ...") AND the exit
                                                # code says so: a driver that gates on rc must not record a hang as success


# ------------------------------------------------------------------ engines
def growmap_for(tree):
    from umbrella_amd.sequoia_utils import DEFAULT_ACC, generate_sequoia_tree
    if tree == "3x4":
        return generate_sequoia_tree(3, 4), DEFAULT_ACC
    if tree == "mi355x-T16d3":
        # growmap re-tuned for the measured MI355X cost ratios (scripts/tune_growmap.py, profiles/r02_growmap_tuning_*.json):
        # the 15 most probable nodes of depth <= 3 under the same acceptance vector -- one draft forward fewer, a full
        # 16-row token tile in the verify
        with open(os.path.join(ROOT, "umbrella_amd", "trees", "mi355x_70b_awq_1b-T16d3.json")) as f:
            return json.load(f), DEFAULT_ACC
    return generate_sequoia_tree(5, 6, ACC_5x6), ACC_5x6


def build_engine(wl, device, dtype, max_length, seed):
    from umbrella_amd.speculation.static_speculation_engine import StaticSpeculationEngine
    gm, acc = growmap_for(wl["tree"])
    eng = StaticSpeculationEngine(wl["draft"], wl["target"], dtype=dtype, device=device, growmap=gm,
                                  max_length=max_length, exit_layer=16, seed=seed)
    eng.initialize()
    return eng, gm, acc


def run_steps(eng, steps):
    toks0 = eng.num_nodes
    for _ in range(steps):
        eng.step()
    return eng.num_nodes - toks0


def kernel_roofline(eng, reps=40):
    """Live HIP-event timing of the target's four layer linears at the verify shape, each through the kernel (and split
    count / epilogue) the model's schedule actually launches, rotating over the layers so weights come from HBM, not
    the 256 MB Infinity Cache.  Events are recorded on the stream the kernels are launched on (torch's current stream)."""
    from umbrella_amd import _lib
    from umbrella_amd.models.llama import ll_plan, to_fm
    m = eng.target_model
    T = eng.tree_size
    ll = getattr(m, "sched", "") == "ll" and not m.fused and T <= 64
    dt = _lib.dtype_code(m.dtype)
    res = {}
    L = m.num_layers
    for key in ("qkv", "o", "gu", "down"):
        lin0 = m.layers[0][key]
        N, K = lin0.N, lin0.K
        x = torch.randn(T, K, device=m.device).to(m.dtype)
        xfm = to_fm(x)
        part = m._bufs["partial"]
        per_launch = (N * K // 2 + (N // 16) * (K // 128) * 64) if lin0.awq else N * K * 2
        h = torch.zeros(T, N, dtype=m.dtype, device=m.device)
        hw = torch.zeros(64 * N, dtype=m.dtype, device=m.device)
        nw = torch.ones(N, dtype=m.dtype, device=m.device)
        ssq = torch.ones(T, max(N // 16, K // 16, 4), dtype=torch.float32, device=m.device)
        act = torch.zeros(64 * max(N // 2, 8), dtype=m.dtype, device=m.device)
        info = {"family": "split-K", "R": lin0.R, "S": lin0.S}
        if ll and key == "gu" and lin0.S == 1 and N // (64 * lin0.R) >= 256:
            # low-latency schedule, large-N gate/up: LDS-shared kernel, FM in / FM out, 1/rms from the sums of squares
            fs = _lib.UmbGemmFused()
            fs.ssq_in, fs.ssq_groups, fs.pad0, fs.ssq_dim, fs.eps, fs.pad1 = ssq.data_ptr(), K // 32, ssq.shape[1], float(K), 1e-5, 3
            launch = lambda ln: _lib.call("umb_gemm_fused", act, xfm, K, ln.w, ln.meta, T, N, K, ln.awq, 1, ln.Rtb, 2, fs, dt)
            info = {"family": "split-K kernel (S=1, FM buffers)", "R": lin0.R, "S": 1}
        elif ll:
            R, WN, WK, NW = ll_plan(N, K, bool(lin0.awq))
            fx = _lib.UmbGemmLL()
            if key in ("o", "down"):
                fx.h, fx.hw, fx.norm_w, fx.ssq_out, fx.ssq_out_stride = h.data_ptr(), hw.data_ptr(), nw.data_ptr(), ssq.data_ptr(), ssq.shape[1]
                epi, out = 4, None
            elif key == "gu":
                fx.ssq_in, fx.ssq_groups, fx.ssq_in_stride, fx.ssq_dim, fx.eps = ssq.data_ptr(), K // 32, ssq.shape[1], float(K), 1e-5
                epi, out = 2, act
            else:
                epi, out = 0, part                      # qkv: the GEMM itself (RoPE / KV append epilogue writes only kilobytes)
            launch = lambda ln: _lib.call("umb_gemm_ll", out, xfm, ln.w, ln.meta, T, N, K, ln.awq, epi, fx, dt)
            info = {"family": "low-latency", "R": R, "WN": WN, "WK": WK}
        else:
            S = lin0.S
            if key in ("o", "down"):                    # model.hip eff_s(): split count of the row-reduced linears
                cap = max(K // 1792, 4)
                if lin0.S_row > 0:
                    S = lin0.S_row
                elif S > cap and (N // (64 * max(lin0.R, 1))) * cap >= 256:
                    S = cap
            epi = 2 if key == "gu" else 0
            out = act if key == "gu" else part
            launch = lambda ln: _lib.call("umb_gemm", out, x, x.stride(0), ln.w, ln.meta, T, N, K, ln.awq, S, ln.Rtb, epi, dt)
            info = {"family": "split-K", "R": lin0.R, "S": S, "tiles_per_block": (lin0.tb & 0x7f) or 4 * lin0.R, "waves_per_block": 8 if lin0.tb & 0x80 else 4}
        for i in range(4):
            launch(m.layers[i % L][key])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(reps):
            launch(m.layers[(i + 4) % L][key])
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / reps
        res[key] = dict(N=N, K=K, bytes=per_launch, us=us, gbs=per_launch / us / 1e3, **info)
    return res


def roofline_block(eng):
    m = eng.target_model
    kr = kernel_roofline(eng)
    dom = max(kr.values(), key=lambda r: r["bytes"])
    tot_b, tot_us = sum(r["bytes"] for r in kr.values()), sum(r["us"] for r in kr.values())
    # HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process, so the figure is
    # the committed result of separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (profiles/README.md); it is
    # only reported while the kernel source it was taken from is unchanged (sha256 of csrc/gemm.hip recorded there)
    traffic, tsrc = None, None
    import hashlib
    with open(os.path.join(ROOT, "umbrella_amd", "csrc", "gemm.hip"), "rb") as f:
        src_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    import glob
    for pmc in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_gemm70b_traffic.json")), reverse=True):   # newest round first
        pmc_name = os.path.basename(pmc)
        if m.config.awq and dom["N"] == 57344 and dom["K"] == 8192 and os.path.exists(pmc):
            with open(pmc) as f:
                rec = json.load(f)
            if rec.get("gemm_hip_sha256_16") == src_hash:      # a figure taken on other kernel source is not reported
                traffic = rec["gate_up_traffic_bytes"]
                tsrc = f"static: profiles/{pmc_name} (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes on this gemm.hip)"
                break
    return {"bound": "hbm", "kernel": f"{dom['family']} {'int4' if m.config.awq else 'dense'} gate_up "
                                      f"N={dom['N']} K={dom['K']} T={eng.tree_size}",
            "achieved": round(dom["gbs"], 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(dom["gbs"] / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": tsrc,
            "avg_launch_us": round(dom["us"], 2), "bytes_per_launch": dom["bytes"],
            "layer_gemms": {k: {kk: (round(vv, 2) if isinstance(vv, float) else vv) for kk, vv in v.items()
                                if kk not in ("N", "K", "bytes")} for k, v in kr.items()},
            "layer_gemms_GBs": round(tot_b / tot_us / 1e3, 1)}


# ------------------------------------------------------------------ CPU baseline (the oracle, rank 0, N = 1 only)
def _oracle_state(cfg, layers, alias):
    """fp32 random state dict for the oracle; with alias=True the `layers` decoder layers share one set of tensors
    (full-depth arithmetic and memory traffic -- a 70B layer is 3.4 GB in fp32, far beyond any cache -- at one
    layer's RAM)."""
    from umbrella_amd.models.synthetic import linear_shapes

    pool = torch.randn((1 << 24) + 12347) * 0.02        # Gaussian entries; the period shares no factor with any row length

    def rnd(n, k):      # every element a Gaussian draw from the pool laid end to end (no two rows equal, no rank-1 structure);
        reps = -(-(n * k) // pool.numel())               # costs one pass over memory instead of 4 G serial mt19937 draws
        return pool.repeat(reps)[:n * k].view(n, k)
    sd = {"model.embed_tokens.weight": rnd(cfg.vocab_size, cfg.hidden_size),
          "model.norm.weight": torch.ones(cfg.hidden_size)}
    if not cfg.tie_word_embeddings:
        sd["lm_head.weight"] = rnd(cfg.vocab_size, cfg.hidden_size)
    first = {}
    for i in range(layers):
        p = f"model.layers.{i}."
        for ln, (n, k) in linear_shapes(cfg).items():
            key = ln + ".weight"
            if not alias or i == 0:
                first[key] = rnd(n, k)
            sd[p + key] = first[key]
        sd[p + "input_layernorm.weight"] = torch.ones(cfg.hidden_size)
        sd[p + "post_attention_layernorm.weight"] = torch.ones(cfg.hidden_size)
    return sd


def cpu_baseline(wl, gm, accept_len, threads):
    """Oracle ("port": torch CPU fp32, AWQ dequantised at load as a CPU port would) MEASURED on the host cores on a bounded
    sample of the same workload (~30-60 s): every draft forward of one static-tree iteration on the full 16-layer draft,
    and the T-row verify on 4 and on 16 of the target's layers (+ lm_head) AFTER a warm-up forward -- the verify of all
    L layers is t(4) + (L - 4) * (t(16) - t(4)) / 12: layers are identical in shape, cost and memory traffic (3.4 GB of
    fp32 weights each, far beyond any cache; the measured layers alias one layer's tensors to fit RAM).  Round 4 timed
    one un-warmed 80-layer forward (96 s, first-touch dominated); the thread counts are on the line.
    tokens/s = accept_len / iteration."""
    import copy
    from oracle.model import OracleLlama
    from umbrella_amd.models.config import KNOWN, rope_inv_freq
    torch.set_num_threads(threads)
    T = gm["size"]
    P = 128

    def build(name, alias, layers=None):
        cfg = copy.copy(KNOWN[name])
        if layers is not None:
            cfg.num_hidden_layers = layers
        sd = _oracle_state(cfg, cfg.num_hidden_layers, alias)
        inv, sc = rope_inv_freq(cfg)
        return OracleLlama(cfg, sd, inv, sc, max_length=256, dtype=torch.float32)

    def forward(m, rows):
        ids = torch.randint(3, 500, (1, rows))
        pos = torch.arange(P, P + rows)[None]
        mk = torch.ones(rows, 256, dtype=torch.bool)
        m.kv_cache.kv_offset = P
        t0 = time.time()
        m.inference(ids, pos, mk, torch.arange(P, P + rows))
        return time.time() - t0

    widths = [len(x) for x in gm["roots"]]
    draft = build(wl["draft"], alias=False)
    forward(draft, 1)                                      # warm the thread pool / allocator
    t_draft = sum(forward(draft, w) for w in widths)       # the reference schedule: one draft forward per level
    del draft
    full_layers = KNOWN[wl["target"]].num_hidden_layers
    if full_layers > 16:
        t16m = build(wl["target"], alias=True, layers=16)
        forward(t16m, T)                                   # warm-up: first touch of the weights and the scratch
        t16 = forward(t16m, T)
        del t16m
        t4m = build(wl["target"], alias=True, layers=4)
        forward(t4m, T)
        t4 = forward(t4m, T)
        del t4m
        per_layer = max(t16 - t4, 0.0) / 12.0
        t_target = t4 + (full_layers - 4) * per_layer
        how = (f"the {T}-row verify measured warm on 4 and on 16 target layers + lm_head ({t4:.2f} s / {t16:.2f} s) and "
               f"extended to all {full_layers} layers at {per_layer:.3f} s per layer")
    else:
        target = build(wl["target"], alias=True)
        forward(target, T)
        t_target = forward(target, T)
        del target
        how = f"the {T}-row verify measured warm through all {full_layers} target layers + lm_head"
    it = t_draft + t_target
    return {"value": round(accept_len / it, 4), "unit": "tokens/s", "cores": threads, "kind": "port",
            "threads": torch.get_num_threads(), "interop_threads": torch.get_num_interop_threads(), "host_cpus": os.cpu_count(),
            "iteration_s": round(it, 3), "draft_s": round(t_draft, 3), "verify_s": round(t_target, 3),
            "sample": f"one static-tree iteration with the oracle (torch CPU fp32): {len(widths)} draft forwards (rows {widths}) "
                      f"on the full draft measured; {how}; context 128; Gaussian weights; target layers alias one layer's fp32 "
                      f"tensors (RAM), same arithmetic and traffic; tokens/s at the GPU run's accept_len {accept_len:.2f}"}


# ------------------------------------------------------------------ the headline configuration at other prompt lengths
def context_sweep(eng, wl, gm, acc, args):
    """synthetic prompts of P in {64, 128, 256, 512} tokens (MT-Bench turn 1 with its system prompt is 70-420).
    The headline is P = 128; here the same engine, tree, acceptance knob and procedure at the other lengths plus one prompt
    that nearly fills max_length -- what the context costs the iteration (tree attention and the KV reads; the weights'
    44 GB do not change).  Bounded step counts; a failure here never takes the headline with it."""
    from umbrella_amd.speculation.steering import steered_measure
    out = {}
    lengths = [64, 256, 512, max(512, min(args.max_length, 2048) - 512)]
    if os.environ.get("UMB_BENCH_CONTEXTS"):                       # experiments: "512,900"
        lengths = [int(v) for v in os.environ["UMB_BENCH_CONTEXTS"].split(",")]
    steps = int(os.environ.get("UMB_BENCH_CONTEXT_STEPS", 16))
    for P in lengths:
        try:
            g = torch.Generator().manual_seed(4321 + P)
            prompt = torch.randint(3, wl.get("vocab_hi", 128000), (1, P), generator=g)
            eng.reset()
            r = steered_measure(eng, prompt, acc, args.seed, 4, steps, len(gm["roots"]))
            out[str(P)] = {"ms_per_step": r["ms_per_step"], "accept_len": r["accept_len"],
                           "tokens_per_s": r["tokens_per_s"]}
        except Exception as e:
            out[str(P)] = {"error": f"{type(e).__name__}: {e}"}
    try:
        eng.reset()
    except Exception:
        pass
    return out


# ------------------------------------------------------------------ secondary configurations (BASELINE configs 2-4), N = 1
def _timed_steps(eng, prompt, warm, steps):
    assert eng._prefill(prompt)
    for _ in range(warm):
        eng.step()
    torch.cuda.synchronize()
    start, t0 = eng.num_nodes, time.time()
    for _ in range(steps):
        eng.step()
    torch.cuda.synchronize()
    dt = time.time() - t0
    return dt / steps * 1e3, (eng.num_nodes - start) / steps


def _event_ms(fn, reps=3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def secondary_configs(device, seed=0):
    """BASELINE configs 2-4 on this GPU with bounded step counts (raw random-weight draft: accept ~1, so only
    `ms_per_step` and the rates are meaningful), each with the figure that bounds it: C2 HBM GB/s, C3-resident and C4
    dense MFMA TFLOP/s of the verify forward, C3-offload host-link GB/s at num_cache_layers 0 and 40."""
    from umbrella_amd.models import AutoModelLM
    from umbrella_amd.sequoia_utils import generate_sequoia_tree
    from umbrella_amd.speculation.auto_engine import AutoEngine
    out = {}
    prompt = torch.randint(3, 128000, (1, 128), generator=torch.Generator().manual_seed(0))

    def guarded(name, fn):
        t0 = time.time()
        try:
            out[name] = fn()
        except Exception as e:                                  # a secondary line never takes the headline with it
            out[name] = {"error": f"{type(e).__name__}: {e}"}
        out[name]["wall_s"] = round(time.time() - t0, 1)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()

    def c2():
        eng = AutoEngine.from_config(device, engine="static", model="meta-llama/Llama-3.1-8B-Instruct", draft_model=D1B,
                                     dtype=torch.bfloat16, growmap=generate_sequoia_tree(5, 6, ACC_5x6), max_length=2048,
                                     exit_layer=16, seed=seed)
        eng.initialize()
        ms, acc = _timed_steps(eng, prompt, 3, 24)
        m, d = eng.target_model, eng.draft_model
        n_fwd = len(eng.levels) - 1 if eng.lookback else len(eng.levels)
        b = n_fwd * d.weight_bytes() + m.weight_bytes()
        return {"config": "C2: Llama-3.1-8B bf16 target + 1B draft, static Sequoia 5x6 (T=31), on-device", "ms_per_step": round(ms, 3),
                "accept_len_raw_draft": round(acc, 2), "iter_bytes_GB": round(b / 1e9, 2), "bound": "hbm",
                "achieved_GBs": round(b / ms / 1e6, 1), "frac": round(b / ms / 1e6 / HBM_PEAK_GBS, 4)}

    shared = {}

    def target70(max_length=4096):
        if "t" not in shared:
            t = AutoModelLM.from_pretrained(T70, max_length=max_length, device=device, dtype=torch.float16, seed=seed)
            t.alloc()
            shared["t"] = t
        return shared["t"]

    def pmc_mfma_busy(T):
        """MFMA-busy of the wide verify GEMM from a COMMITTED counter pass (PMC cannot be read from inside the timed process:
        scripts/r6/pmc_mfma.sh -> profiles/, summarised by scripts/pmc_mfma_busy.py).  Reported only while the kernel sources the
        pass ran on are the tree's (sha256/16 of csrc/gemm.hip and csrc/vgemm.hip recorded in the file); otherwise null."""
        import glob
        import hashlib
        def h(f):
            with open(os.path.join(ROOT, "umbrella_amd", "csrc", f), "rb") as fh:
                return hashlib.sha256(fh.read()).hexdigest()[:16]
        want = {"gemm_hip_sha256_16": h("gemm.hip"), "vgemm_hip_sha256_16": h("vgemm.hip")}
        for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_verify_gemm_T{769 if T > 512 else 256}_mfma_busy.json")), reverse=True):
            try:
                with open(path) as f:
                    rec = json.load(f)
            except Exception:
                continue
            if any(rec.get(k) != v for k, v in want.items()):
                continue                                   # taken on other kernel source: not this build's figure
            ks = [k for k in rec["kernels"] if ("vgemm_w_kernel" in k["kernel"] or "verify_gemm" in k["kernel"]) and "mfma_busy" in k]
            return {"source": f"profiles/{os.path.basename(path)} (committed rocprofv3 --pmc pass on this build's gemm.hip / vgemm.hip, "
                              "not measured by this run)", "by_blocks": {str(k["blocks"]): k["mfma_busy"] for k in ks}}
        return None

    def verify_rate(eng):
        """dense MFMA rate of the verify forward alone (events on the launch stream), 2 T (layer + head parameters) flops"""
        t = eng.target_model
        ms = _event_ms(eng._verify_forward)
        params = sum(ln.N * ln.K for ln in t.layers[0].values()) * t.num_layers + t.lm_head.N * t.lm_head.K
        tf = 2.0 * eng.tree_size * params / (ms * 1e-3) / 1e12
        # `frac` is against the 2.5 PF datasheet peak.  On random fp16 operands a PURE matrix loop sustains 1.85 PF on this part (the
        # power limit, profiles/r06_mfma_power_probe.txt): the second fraction is against that measured ceiling.
        return {"verify_ms": round(ms, 2), "verify_TFLOPs": round(tf, 1), "bound": "mfma",
                "frac": round(tf / MFMA_PEAK_TFLOPS, 4), "frac_of_random_data_mfma_ceiling_1850TF": round(tf / 1850.0, 4),
                "mfma_busy": pmc_mfma_busy(eng.tree_size)}

    def c3_resident():
        t = target70()
        d = AutoModelLM.from_pretrained(D1B, max_length=t.max_length, device=device, dtype=torch.float16, seed=seed)
        d.alloc()
        eng = AutoEngine.from_config(device, engine="dynamic", model=T70, draft_model=D1B, dtype=torch.float16, width=16,
                                     num_beams=24, depth=16, max_length=t.max_length, offload=False, target_model_obj=t,
                                     draft_model_obj=d, seed=seed)
        eng.initialize()
        ms, acc = _timed_steps(eng, prompt, 2, 8)
        r = {"config": "C3 with the target resident: 70B-AWQ + 1B draft, dynamic w16/b24/d16 (T=257)", "ms_per_step": round(ms, 2),
             "accept_len_raw_draft": round(acc, 2)}
        r.update(verify_rate(eng))
        eng.reset()
        return r

    def c4():
        t = target70()
        d = AutoModelLM.from_pretrained(D8BAWQ, max_length=t.max_length, device=device, dtype=torch.float16, seed=seed)
        d.alloc()
        eng = AutoEngine.from_config(device, engine="dynamic", model=T70, draft_model=D8BAWQ, dtype=torch.float16, width=32,
                                     num_beams=32, depth=24, max_length=t.max_length, offload=False, temperature=0.6, topp=0.9,
                                     topk=32, repetition_penalty=1.05, target_model_obj=t, draft_model_obj=d, seed=seed)
        eng.initialize()
        ms, acc = _timed_steps(eng, prompt, 1, 4)
        r = {"config": "C4: 70B-AWQ + 8B-AWQ draft, dynamic w32/b32/d24 (T=769), stochastic (T 0.6, top-p 0.9, top-k 32, "
                       "penalty 1.05)", "ms_per_step": round(ms, 2), "accept_len_raw_draft": round(acc, 2)}
        r.update(verify_rate(eng))
        eng.reset()
        return r

    def prefill():
        t = target70()
        ids = torch.randint(3, 128000, (2048,), generator=torch.Generator().manual_seed(1)).int().to(device)
        t.reserve(t.PREFILL_CHUNK, logit_rows=64)
        t.clear(); t.prefill_tokens(ids, 0); torch.cuda.synchronize()
        t.clear(); t0 = time.time(); t.prefill_tokens(ids, 0); torch.cuda.synchronize()
        dt = time.time() - t0
        t.clear()
        params = sum(ln.N * ln.K for ln in t.layers[0].values()) * t.num_layers
        tf = 2.0 * 2048 * params / dt / 1e12
        return {"config": "70B-AWQ prompt of 2048 tokens, 1024-token chunks", "tok_s": round(2048 / dt, 0), "ms": round(dt * 1e3, 1),
                "TFLOPs": round(tf, 1), "bound": "mfma", "frac": round(tf / MFMA_PEAK_TFLOPS, 4)}

    def c3_offload(ncl):
        def run():
            eng = AutoEngine.from_config(device, engine="dynamic", model=T70, draft_model=D1B, dtype=torch.float16, width=16,
                                         num_beams=24, depth=16, max_length=4096, offload=True, num_cache_layers=ncl, seed=seed)
            eng.initialize()
            # STEADY STATE, as generation runs it: step() ends with a synchronize of the LAUNCH stream only (the accept result), so
            # the next verify's first slabs keep crossing the link while the host decides and the next draft tree runs.  Rounds
            # 2-5 timed every step between two DEVICE-wide synchronizes, which also drain the copy stream: each timed step then
            # began with a full slab ring and an idle link for the whole draft + resident-prefix phase (~36 ms at 40 resident
            # layers) -- 356 ms per step where the link's 40 back-to-back copies take 318 (profiles/r06_offload_copy_profile.txt).
            # Both figures are reported; `ms_per_step` is the steady one over 5 consecutive steps, one clock around them.
            assert eng._prefill(prompt)
            for _ in range(2):
                eng.step()
            start = eng.num_nodes
            t0 = time.time()
            nst = 5
            for _ in range(nst):
                eng.step()                              # (ends with current_stream().synchronize(): the step's tokens are final)
            ms = (time.time() - t0) * 1e3 / nst
            acc = (eng.num_nodes - start) / nst
            torch.cuda.synchronize()
            times = []
            for _ in range(3):                          # the old way, for continuity: every step between device-wide synchronizes
                t0 = time.time()
                eng.step()
                torch.cuda.synchronize()
                times.append((time.time() - t0) * 1e3)
            m = eng.target_model
            streamed = sum(1 for h in m.host_slabs if h is not None) * m.slab_bytes
            torch.cuda.synchronize()
            place = m.host_placement()
            return {"config": f"C3: 70B-AWQ layers streamed from pinned host DRAM, num_cache_layers {ncl}, 1B draft, dynamic "
                              "w16/b24/d16 (T=257)", "ms_per_step": round(ms, 1), "accept_len_raw_draft": round(acc, 2),
                    "streamed_GB_per_verify": round(streamed / 1e9, 2), "bound": "host link (PCIe Gen5 x16, 63 GB/s spec)",
                    "achieved_GBs": round(streamed / ms / 1e6, 1), "frac": round(streamed / ms / 1e6 / 63.0, 4),
                    "steady_steps": nst, "step_ms_device_synced": [round(t, 1) for t in times], "host": place}
        return run

    guarded("c2", c2)
    guarded("c3_resident", c3_resident)
    guarded("c4", c4)
    guarded("prefill_70b", prefill)
    shared.clear()
    torch.cuda.empty_cache()
    def fresh_host():
        # Every offload configuration pins fresh host memory, as a process running it alone does (torch caches pinned blocks).
        # (Rounds 3-5 chased a 330 / 357 / 377 ms spread of the 40-resident-layer figure through NUMA placement; it was the
        # per-step device-wide synchronize of this script -- see c3_offload.)
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        if hasattr(torch._C, "_host_emptyCache"):
            torch._C._host_emptyCache()
    fresh_host()
    guarded("c3_offload_ncl0", c3_offload(0))
    fresh_host()
    guarded("c3_offload_ncl40", c3_offload(40))
    fresh_host()
    return out


# ------------------------------------------------------------------ the headline loop (per rank)
def headline(args, wl, dtype, device, rank, world, dist, agg_device):
    eng, gm, acc = build_engine(wl, device, dtype, args.max_length, args.seed + rank)
    g = torch.Generator().manual_seed(1234 + rank)
    prompt = torch.randint(3, wl.get("vocab_hi", 128000), (1, args.prompt_len), generator=g)           # examples/bench.py:31

    # ---- untimed: the target's own greedy continuation (ground truth for the acceptance knob)
    need = (args.warmup + args.steps) * len(gm["roots"]) + 16
    from umbrella_amd.speculation.steering import disable_eos
    disable_eos(eng)                  # random-init logits: an accepted EOS id would end the request inside the timed loop
    assert eng._prefill(prompt)
    start = eng.num_nodes
    torch.cuda.synchronize()
    t0 = time.time()
    raw_steps = 0
    while eng.num_nodes - start < need and eng.validate_status():
        eng.step()
        raw_steps += 1
    torch.cuda.synchronize()
    raw_dt = time.time() - t0
    raw_tokens = eng.num_nodes - start
    truth = eng.tokens[start:eng.num_nodes + 1].tolist()
    raw_tps = raw_tokens / raw_dt
    raw_accept = raw_tokens / max(raw_steps, 1)

    # A token verified as a depth-d tree node sums its attention in a different order than the same token
    # verified as a root, so on random-init weights a 16-bit near-tie can flip the target's arg-max about
    # once per ~50 tokens and leave the recorded continuation.  The kernels are deterministic, so the
    # continuation is re-recorded under the knob's own execution pattern until it is a fixed point
    # (each pass reproduces the previous one bit-for-bit up to its first divergence).
    passes = 0
    max_passes = max(8, min(40, (args.warmup + args.steps + 15) // 16))   # ~1 near-tie flip per 50 tokens: long runs need more
    for passes in range(1, max_passes + 1):
        eng.reset()
        assert eng._prefill(prompt)
        eng.set_oracle_draft(truth, start, acc, seed=args.seed)
        run_steps(eng, args.warmup + args.steps)
        div = eng.diverged
        while eng.num_nodes - start < need and eng.validate_status():
            eng.step()
        new_truth = eng.tokens[start:eng.num_nodes + 1].tolist()
        if div == 0:
            break
        truth = new_truth

    # ---- timed: acceptance knob on
    eng.reset()
    assert eng._prefill(prompt)
    eng.set_oracle_draft(truth, start, acc, seed=args.seed)
    run_steps(eng, args.warmup)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.time()
    tokens = run_steps(eng, args.steps)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.time() - t0
    dt, tokens = aggregate(dt, tokens, world, dist, agg_device)
    info = dict(start=start, raw_tps=raw_tps, raw_accept=raw_accept, passes=passes, head=[int(t) for t in truth[:8]])
    return eng, gm, acc, dt, tokens, info


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(eng, start, out_dir):
    """--dump-outputs: what the timed loop computed in its LAST step, as a caller of the engine receives it, written as
    .npy files so that two builds can be compared output for output (the same arguments give the same seeded weights,
    prompt and acceptance draws):
      tokens.npy            the request's emitted ids from the end of the prompt through that step (what generate()
                            returns: the bonus token last), float64
      last_step_tokens.npy  the ids that step committed, its bonus token last, float64
      target_logits.npy     the target's verify logits of that step, [tree_size, vocab], float32
    Must run right after the timed loop, before anything else uses the engine."""
    import numpy as np
    torch.cuda.synchronize()
    n, keep = eng.num_nodes, eng.last_accept
    toks = eng.tokens[:n + 1].to(torch.float64).cpu()
    arrays = {"tokens": toks[start:], "last_step_tokens": toks[n - keep:],
              "target_logits": eng.target_model.logits_buffer[:eng.tree_size, :eng.vocab_size].float().cpu()}
    total = sum(a.numel() * a.element_size() for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a.numpy())
    return {"dir": out_dir, "shapes": {name: list(a.shape) for name, a in arrays.items()}}


def aggregate(dt, tokens, world, dist, agg_device):
    """max over ranks of the timed region, sum over ranks of the units processed"""
    if world > 1:
        tt = torch.tensor([dt, float(tokens)], dtype=torch.float64, device=agg_device)
        mx = tt.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        dist.all_reduce(tt, op=dist.ReduceOp.SUM)
        dt, tokens = float(mx[0]), float(tt[1])
    return dt, tokens


def headline_line(args, wl, eng, gm, acc, dt, tokens, info, world):
    m, d = eng.target_model, eng.draft_model
    levels = [len(x) for x in gm["roots"]]
    accept_len = tokens / (args.steps * world)
    n_mid = info["start"] + tokens / world / 2
    kv_t = m.num_layers * 2 * m.config.num_key_value_heads * m.config.head_dim * 2
    kv_d = d.num_layers * 2 * d.config.num_key_value_heads * d.config.head_dim * 2
    # draft forwards actually executed per iteration: one per expanded level (the reference's extra KV-fill
    # forward over the deepest level is folded into the next root forward, engine_common._draft_root), each
    # with its lm_head; without the look-back the reference count (len(levels), last one without lm_head)
    if getattr(eng, "lookback", False):
        n_fwd = len(levels) - 1
        draft_fwd = d.weight_bytes()
    else:
        n_fwd = len(levels)
        draft_fwd = d.weight_bytes() - (d.lm_head.N * d.lm_head.K * 2) / len(levels)
    bytes_iter = n_fwd * draft_fwd + m.weight_bytes() + n_mid * (kv_t + n_fwd * kv_d)
    iter_ms = dt / args.steps * 1e3
    return {"metric": "tokens/s @ bs=1 (speculative decoding)", "value": round(tokens / dt, 2), "unit": "tokens/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(iter_ms, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": wl["dtype"],
            "data": "synthetic: random-init weights of the exact shapes, random prompt ids; acceptance set by the "
                    "controllable-acceptance draft (acc vector below), all draft/verify kernels execute",
            "config": {"workload": wl["desc"], "engine": "static", "tree": wl["tree"], "tree_size": eng.tree_size,
                       "prompt_len": args.prompt_len, "max_length": args.max_length, "acc": acc,
                       "parallelism": "1 engine per GPU (replicas: independent requests, no data-path collective)"
                       if world > 1 else "single GPU"},
            "accept_len": round(accept_len, 3), "value_raw_draft": round(info["raw_tps"], 2),
            "accept_len_raw_draft": round(info["raw_accept"], 3), "oracle_draft_divergence": getattr(eng, "diverged", 0),
            "oracle_draft_passes": info["passes"], "continuation_head": info["head"], "schedule": getattr(m, "sched", "split"),
            "draft_forwards_per_iter": n_fwd, "iter_bytes_GB": round(bytes_iter / 1e9, 3),
            "iter_hbm_frac": round(bytes_iter / (iter_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}


def dry_run(args, rank, world, dist):
    """Launch-plumbing check without a GPU (tests): the ranks come up over gloo, the timed region is a sleep, the
    aggregation (barriers, max over ranks, sum of units) and the one-line report are the real code."""
    if world > 1:
        dist.barrier()
    t0 = time.time()
    for _ in range(args.steps):
        time.sleep(0.002 * (1 + rank))
    tokens = 3 * args.steps
    if world > 1:
        dist.barrier()
    dt, tokens = aggregate(time.time() - t0, tokens, world, dist, "cpu")
    return {"metric": "tokens/s @ bs=1 (speculative decoding)", "value": round(tokens / dt, 2), "unit": "tokens/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "none", "dry_run": True,
            "data": "DRY RUN: no GPU work, launch plumbing only", "config": {"workload": "dry run"},
            "accept_len": round(tokens / (args.steps * world), 3), "pp": {"skipped": "dry run"}, "tp": {"skipped": "dry run"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workload", default="70b-awq+1b", choices=sorted(WORKLOADS))
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--max-length", type=int, default=2048)
    ap.add_argument("--tree", default=None, choices=[None, "3x4", "5x6", "mi355x-T16d3"],
                    help="growmap override (default: the workload's reference tree); mi355x-T16d3 = the re-tuned tree, a "
                         "second line next to the headline, never the headline itself")
    ap.add_argument("--parallel", default="replicas", choices=["replicas", "pp", "tp"],
                    help="replicas (default): the headline; at N > 1 followed by the pp and tp measurements on the same "
                         "line.  pp / tp: that engine alone (its own line)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip BASELINE configs 2-4 (N = 1)")
    ap.add_argument("--no-sharded", action="store_true", help="skip the pp / tp measurements (N > 1)")
    ap.add_argument("--sharded-steps", type=int, default=16, help="timed iterations of the pp / tp measurements")
    ap.add_argument("--phase-timeout", type=float, default=240.0, help="watchdog per pp / tp phase, seconds")
    ap.add_argument("--dry-run", action="store_true", help="launch plumbing only (gloo, no GPU work)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed (emitted token ids, the target's verify "
                         "logits) to DIR/<name>.npy, rank 0 of the headline")
    args = ap.parse_args()
    if args.dump_outputs and (args.dry_run or args.parallel != "replicas"):
        raise SystemExit("--dump-outputs writes the headline's outputs: not with --dry-run or --parallel pp / tp")
    if os.environ.get("UMB_BENCH_STACKS"):              # diagnostics: dump every thread's Python stack after N seconds
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["UMB_BENCH_STACKS"]), repeat=False)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    # A run of K timed iterations emits up to depth + 1 tokens in each: the reference's max_length 2048 holds ~370 iterations of the
    # 3x4 tree behind a 128-token prompt.  Longer runs get the KV capacity they need (reported as config.max_length) instead of
    # stopping inside the timed loop.
    need_len = args.prompt_len + (args.warmup + args.steps + 4) * 7 + 64
    if need_len > args.max_length:
        args.max_length = (need_len + 1023) // 1024 * 1024
        print(f"bench.py: --steps {args.steps} needs a context of {need_len} tokens: max_length raised to {args.max_length}", file=sys.stderr)
    self_launch(args)                                   # N > 1 outside torch.distributed.run: start N ranks

    rank, world, local = dist_env()
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} but WORLD_SIZE={world}: launch N ranks for --gpus N "
                         "(python -m torch.distributed.run --nproc-per-node N ..., or plain `python bench.py --gpus N`)")
    dist = None
    gloo = args.dry_run or share_gpu()
    if not args.dry_run:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a HIP device (MI355X); use --dry-run for the launch plumbing alone")
        dev_index = 0 if share_gpu() else local
        if torch.cuda.device_count() <= dev_index:
            raise SystemExit(f"rank {rank}: no GPU {dev_index} on this box ({torch.cuda.device_count()} visible): "
                             f"--gpus {args.gpus} needs {args.gpus} devices")
        torch.cuda.set_device(dev_index)
        device = f"cuda:{dev_index}"
    if world > 1 or args.parallel != "replicas":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        if gloo:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(device))
        if dist.get_world_size() != args.gpus:
            raise SystemExit(f"process group has {dist.get_world_size()} ranks, --gpus {args.gpus} asked for")
    if args.dry_run:
        out = dry_run(args, rank, world, dist)
        if rank == 0:
            print(json.dumps(out), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return out

    if args.workload == "tiny":
        register_tiny()
    wl = dict(WORKLOADS[args.workload])
    if args.tree:
        wl["tree"] = args.tree
        wl["desc"] = wl["desc"] + f" [growmap override: {args.tree}]"
    dtype = torch.float16 if wl["dtype"] == "fp16" else torch.bfloat16
    agg_device = "cpu" if gloo else device

    if args.parallel == "pp":
        from umbrella_amd.parallel import run_pp_bench
        return run_pp_bench(args, wl, dtype, device, rank, world)
    if args.parallel == "tp":
        from umbrella_amd.tensor_parallel import run_tp_bench
        return run_tp_bench(args, wl, dtype, device, rank, world)

    import __graft_entry__ as ge
    ge.build()
    if world == 1 and not args.no_secondary and args.workload == "70b-awq+1b":
        # the offload legs' host arena is claimed NOW -- NUMA-local to the GPU, one pinned registration -- before the
        # headline's allocations fragment the host (umbrella_amd/models/host_arena.py)
        try:
            from umbrella_amd.models import host_arena
            from umbrella_amd.models.config import KNOWN
            from umbrella_amd.models.llama import PackedLinear
            from umbrella_amd.models.synthetic import linear_shapes
            c70 = KNOWN[T70]
            sh = linear_shapes(c70)
            groups = (("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), ("self_attn.o_proj",),
                      ("mlp.gate_proj", "mlp.up_proj"), ("mlp.down_proj",))
            slab = sum(sum(PackedLinear.packed_bytes(sum(sh[n][0] for n in names), sh[names[0]][1], True)) for names in groups)
            slot = (slab + host_arena.ALIGN - 1) // host_arena.ALIGN * host_arena.ALIGN
            host_arena.reserve(c70.num_hidden_layers * slot, device)
        except Exception as e:                                            # the legs fall back to per-layer pinned tensors
            print(f"bench: host arena not reserved ({type(e).__name__}: {e})", file=sys.stderr, flush=True)
    eng, gm, acc, dt, tokens, info = headline(args, wl, dtype, device, rank, world, dist, agg_device)
    out = headline_line(args, wl, eng, gm, acc, dt, tokens, info, world)
    if args.dump_outputs and rank == 0:
        out["dump_outputs"] = dump_outputs(eng, info["start"], args.dump_outputs)
    accept_len = out["accept_len"]

    if world == 1:
        if not args.no_roofline:
            out["roofline"] = roofline_block(eng)
        if not args.no_secondary and args.workload == "70b-awq+1b":
            out["context_sweep"] = context_sweep(eng, wl, gm, acc, args)
        del eng
        torch.cuda.empty_cache()
        if not args.no_secondary and args.workload == "70b-awq+1b" and not args.tree:
            # a labelled SECOND line next to the headline, never the headline itself: the same workload, acceptance vector, seed,
            # steps and timing method on the growmap re-tuned for MI355X cost ratios (umbrella_amd/trees/mi355x_70b_awq_1b-T16d3.json,
            # scripts/tune_growmap.py: 15 nodes of depth <= 3 -- one draft forward fewer, a full 16-row verify tile)
            try:
                wl2 = dict(wl, tree="mi355x-T16d3", desc=wl["desc"] + " [growmap: mi355x-T16d3]")
                e2, gm2, acc2, dt2, tok2, info2 = headline(args, wl2, dtype, device, rank, world, dist, agg_device)
                l2 = headline_line(args, wl2, e2, gm2, acc2, dt2, tok2, info2, world)
                out["tuned_tree_line"] = {k: l2[k] for k in ("value", "unit", "ms_per_step", "accept_len", "value_raw_draft",
                                                              "draft_forwards_per_iter", "iter_bytes_GB", "iter_hbm_frac")}
                out["tuned_tree_line"].update({"tree": "mi355x-T16d3", "tree_size": e2.tree_size,
                                               "vs_headline_tokens_per_s": round(l2["value"] / out["value"], 4),
                                               "note": "same acceptance vector and seed as the headline; the headline stays on "
                                                       "the reference's 3x4 tree"})
                del e2
            except Exception as e:
                out["tuned_tree_line"] = {"error": f"{type(e).__name__}: {e}"}
            torch.cuda.empty_cache()
        if not args.no_secondary and args.workload == "70b-awq+1b":
            out["secondary"] = secondary_configs(device, args.seed)
        if not args.no_cpu_baseline and args.workload != "tiny":          # the CPU leg runs on rank 0 at N = 1 only
            try:
                out["cpu_baseline"] = cpu_baseline(wl, gm, accept_len, torch.get_num_threads())
            except Exception as e:                                        # never lose the GPU line to the baseline leg
                out["cpu_baseline"] = {"value": None, "unit": "tokens/s", "cores": os.cpu_count(), "kind": "port",
                                       "sample": f"failed: {type(e).__name__}: {e}"}
        print(json.dumps(out), flush=True)
        return out

    # ---- N > 1: the sharded engines, ONE request over all N GPUs each, on the same line
    del eng
    torch.cuda.empty_cache()
    printed = threading.Event()

    def emit(err=None):
        if printed.is_set():
            return
        printed.set()
        # "status" is what a driver gates on: the watchdog exits 0 so that the (complete, valid) headline of this line is
        # not lost with a hung pp / tp phase, and says so here instead of in the exit code
        out["status"] = "ok" if not err else f"sharded phase failed: {err}"
        if err:
            out["sharded_error"] = err
            out.setdefault("pp", {"error": err})
            out.setdefault("tp", {"error": err})
        print(json.dumps(out), flush=True)

    if args.no_sharded:
        out["pp"] = out["tp"] = {"skipped": "--no-sharded"}
    else:
        wd = Watchdog(rank, emit)
        sargs = argparse.Namespace(**vars(args))
        sargs.steps, sargs.warmup = args.sharded_steps, max(2, min(args.warmup, 4))
        for name, mod, fn in (("pp", "umbrella_amd.parallel", "pp_measure"), ("tp", "umbrella_amd.tensor_parallel", "tp_measure")):
            wd.arm(name, args.phase_timeout)
            try:
                import importlib
                r = getattr(importlib.import_module(mod), fn)(sargs, wl, dtype, device, rank, world)
                if rank == 0:
                    out[name] = r
                    # a mis-bound launch (several ranks on one physical device) must not pass for an N-GPU measurement
                    if r and not share_gpu() and r.get("n_distinct_devices") != world:
                        out[name]["error"] = (f"{r.get('n_distinct_devices')} distinct devices behind {world} ranks: "
                                              "not an N-GPU measurement")
            except Exception as e:      # an exception on one rank may leave the others in a collective: the watchdog ends them
                import traceback
                traceback.print_exc()
                out[name] = {"error": f"{type(e).__name__}: {e}"}
            torch.cuda.synchronize()
            dist.barrier()
            torch.cuda.empty_cache()
        wd.disarm()
    if rank == 0:
        emit()
    dist.barrier()
    # The line is out and every rank has passed the barrier.  Ordered teardown: the tp / pp measurements dropped their graphs and
    # peer buffers when they returned (tensor_parallel.shutdown_tensor_parallel); what is left is the drain and the group.  Round 5
    # left through os._exit(0) here because destroying a communicator whose collectives sat in live hipGraphs aborted now and then;
    # tests/test_tensor_parallel.py::test_tp_rccl_hook_inside_the_iteration_graph now loops that teardown and checks the exit code.
    sys.stdout.flush(); sys.stderr.flush()
    import gc
    gc.collect()
    if not args.dry_run:
        torch.cuda.synchronize()
    if os.environ.get("UMB_BENCH_HARD_EXIT") == "1":      # escape hatch only (default off): leave without tearing RCCL down
        os._exit(0)
    dist.destroy_process_group()
    return out


if __name__ == "__main__":
    main()
