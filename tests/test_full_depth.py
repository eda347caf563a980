"""Full-depth engines at the real BASELINE shapes (GPU): config 2 (Llama-3.1-8B bf16 target + Llama-3.2-1B draft, static
Sequoia 5x6) and the headline pairing (Llama-3.1-70B-Instruct-AWQ-INT4 target + 1B draft, static 3x4, fp16), every
layer of every model, seeded random-init weights of the exact shapes (no checkpoints offline).

No CPU oracle finishes an 80-layer 70B forward in test time, so parity is stated through the size-independent properties
the domain offers:
  (1) hipGraph replay == eager launches, token for token;
  (2) greedy speculative decoding == greedy autoregressive decoding with the target alone (T = 1 forwards): every
      emitted token is the arg-max of the autoregressive row that precedes it (teacher forced along the emitted sequence);
      the only accepted exception is a row whose top-2 logit margin lies inside the 16-bit noise band (the GEMMs are
      batch invariant, tree attention sums keys in a different order than a 1-row forward);
  (3) the same with the tree really exercised: the controllable-acceptance draft (bench.py's knob) places the target's
      own continuation in the tree, accept length > 2, tokens still == AR.
"""
import json
import os

import pytest
import torch

from conftest import report_fact

pytestmark = pytest.mark.gpu

NEW = 40
TOL = {torch.bfloat16: 0.35, torch.float16: 0.06}

# Positions at which the speculative decode may differ from the target's own autoregressive arg-max: a COMMITTED list
# (tests/golden/full_depth_near_ties.json, recorded on an MI355X with UMB_RECORD_NEAR_TIES=1; kernels and seeded weights
# are deterministic, so the list is a property of the build).  A miss outside the list fails the test even when it sits
# inside the 16-bit noise band: a build that moves from 0 to 3 near-tie flips has to say so by updating the list.
_TIES_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "full_depth_near_ties.json")
_TIES = json.load(open(_TIES_FILE)) if os.path.exists(_TIES_FILE) else {}
_RECORDED = {}


def _check_allowed(what, misses, n, exact):
    """misses: [[position, emitted token, autoregressive arg-max], ...]"""
    report_fact(f"full_depth/{what}", {"tokens": n, "exact_argmax": exact, "near_tie_positions": misses})
    if os.environ.get("UMB_RECORD_NEAR_TIES"):
        _RECORDED[what] = misses
        out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpurun_out")
        os.makedirs(out, exist_ok=True)
        json.dump(_RECORDED, open(os.path.join(out, "full_depth_near_ties.json"), "w"), indent=1, sort_keys=True)
        return
    allowed = [tuple(m) for m in _TIES.get(what, [])]
    extra = [m for m in misses if tuple(m) not in allowed]
    assert not extra, (f"{what}: {len(extra)} token(s) differ from the autoregressive arg-max at positions that "
                       f"tests/golden/full_depth_near_ties.json does not list: {extra} (exact {exact} of {n})")


def _ar(target, prompt, n, dev):
    """greedy decode with the target alone (T = 1 forwards)"""
    target.clear()
    row = target.prefill_tokens(torch.tensor(prompt, dtype=torch.int32, device=dev), 0)
    toks = []
    for i in range(n):
        toks.append(int(row.argmax()))
        if i + 1 < n:
            row = target.prefill_tokens(torch.tensor([toks[-1]], dtype=torch.int32, device=dev), len(prompt) + i)
    target.clear()
    return toks


def _check_against_ar(target, prompt, toks, tol, dev, what):
    """Teacher-forced autoregressive check: the target alone walks prompt + toks one token per forward; token i must be
    the arg-max of the row that precedes it.  Where that row's top-2 margin is inside the 16-bit noise band (2 tol) the
    speculative decode may have taken the runner-up (tree attention sums keys in another order) -- it must then be
    within 2 tol of the maximum.  Returns the number of exact arg-max agreements."""
    target.clear()
    row = target.prefill_tokens(torch.tensor(prompt, dtype=torch.int32, device=dev), 0)
    exact, misses = 0, []
    for i, tok in enumerate(toks):
        top2 = row.topk(2).values
        best, margin, gap = int(row.argmax()), float(top2[0] - top2[1]), float(top2[0] - row[tok])
        if tok == best:
            exact += 1
        else:
            assert margin < 2 * tol and gap < 2 * tol, \
                f"{what}: token {i} = {tok} is not the autoregressive choice {best} (margin {margin:.4f}, gap {gap:.4f})"
            misses.append([i, int(tok), best])
        if i + 1 < len(toks):
            row = target.prefill_tokens(torch.tensor([tok], dtype=torch.int32, device=dev), len(prompt) + i)
    target.clear()
    _check_allowed(what, misses, len(toks), exact)
    return exact


def _run_pair(target_name, draft_name, dtype, tree, acc, dev, tag):
    from umbrella_amd.models import AutoModelLM
    from umbrella_amd.sequoia_utils import DEFAULT_ACC, generate_sequoia_tree
    from umbrella_amd.speculation.speculation_utils import IdTokenizer
    from umbrella_amd.speculation.static_speculation_engine import StaticSpeculationEngine
    L = 512
    target = AutoModelLM.from_pretrained(target_name, max_length=L, device=str(dev), dtype=dtype)
    target.alloc()
    draft = AutoModelLM.from_pretrained(draft_name, max_length=L, device=str(dev), dtype=dtype, cuda_graph=True)
    draft.alloc(exit_layer=16)
    assert target.num_layers == target.config.num_hidden_layers and draft.num_layers == draft.config.num_hidden_layers
    gm = generate_sequoia_tree(*tree) if acc is None else generate_sequoia_tree(*tree, acc)
    acc = DEFAULT_ACC if acc is None else acc
    prompt = torch.randint(3, 128000, (96,), generator=torch.Generator().manual_seed(1)).tolist()

    def engine(graph):
        e = StaticSpeculationEngine(draft_name, target_name, dtype=dtype, device=str(dev), growmap=gm, max_length=L,
                                    draft_model_obj=draft, target_model_obj=target, tokenizer=IdTokenizer(), hip_graph=graph)
        e.initialize()
        return e

    eg, ee = engine(True), engine(False)
    tol = TOL[dtype]
    ar = _ar(target, prompt, NEW + 16, dev)                             # after initialize(): the workspaces are final
    out_g = eg.generate(input_ids=prompt, max_new_tokens=NEW)
    out_e = ee.generate(input_ids=prompt, max_new_tokens=NEW)
    tg, te = out_g["generated_tokens"], out_e["generated_tokens"]
    assert tg == te, "hipGraph replay and eager launches disagree"
    assert len(tg) >= NEW
    exact = _check_against_ar(target, prompt, tg, tol, dev, f"{tag}/raw draft")
    # (3) the tree exercised: the target's own continuation steered into the tree.  A token verified as a depth-d tree
    # node sums its attention in another order than the same token verified as a root, so a 16-bit near-tie can move
    # the steered run off the recorded continuation (after which nothing is accepted any more): as bench.py does, the
    # continuation is re-recorded under the knob's own execution pattern until it is a fixed point.
    truth = ar
    for _ in range(8):
        assert eg._prefill(torch.tensor([prompt]))
        start = eg.num_nodes
        eg.set_oracle_draft(truth, start, acc, seed=0)
        steps = 0
        while eg.num_nodes - start < NEW and eg.validate_status():
            eg.step()
            steps += 1
        accept = (eg.num_nodes - start) / max(steps, 1)
        div = eg.diverged
        while eg.num_nodes - start < NEW + 16 and eg.validate_status():
            eg.step()
        tk = eg.tokens[start:start + NEW + 1].tolist()
        truth = eg.tokens[start:eg.num_nodes + 1].tolist()
        eg.reset()
        if div == 0:
            break
    assert div == 0, "the steered continuation never became a fixed point"
    exactk = _check_against_ar(target, prompt, tk, tol, dev, f"{tag}/steered draft")
    same = next((i for i in range(min(len(tg), len(ar))) if tg[i] != ar[i]), min(len(tg), len(ar)))
    return dict(n=len(tg), exact=exact, nk=len(tk), exactk=exactk, accept=accept, same_as_free_ar=same,
                raw_accept=out_g["avg_accept_tokens"])


def _assert_pair(r):
    # at most a handful of 16-bit near-ties in 40+ tokens (each one margin-checked above), the rest exact
    assert r["n"] >= NEW and r["exact"] >= r["n"] - 3, r
    assert r["nk"] >= NEW and r["exactk"] >= r["nk"] - 3, r
    assert r["accept"] > 2.0, r
    report_fact("full_depth/pair summary " + str(r["n"]) + " tokens", r)


def test_c2_8b_bf16_with_1b_draft_5x6():
    """BASELINE config 2: Llama-3.1-8B-Instruct target + Llama-3.2-1B draft, bf16, static Sequoia 5x6 (T = 31), all 32 + 16
    layers.  8B target on the split schedule, 1B draft on the low-latency one (UMB_SCHED=auto)."""
    dev = torch.device("cuda:0")
    r = _run_pair("meta-llama/Llama-3.1-8B-Instruct", "meta-llama/Llama-3.2-1B-Instruct", torch.bfloat16, (5, 6),
                  [0.5, 0.2, 0.12, 0.08, 0.05, 0.03], dev, "C2 8B + 1B 5x6")
    _assert_pair(r)


def test_70b_awq_with_1b_draft_3x4():
    """The headline pairing at full depth: 80 AWQ int4 layers + 16 draft layers, static 3x4 (T = 13), fp16."""
    dev = torch.device("cuda:0")
    r = _run_pair("hugging-quants/Meta-Llama-3.1-70B-Instruct-AWQ-INT4", "meta-llama/Llama-3.2-1B-Instruct",
                  torch.float16, (3, 4), None, dev, "headline 70B-AWQ + 1B 3x4")
    _assert_pair(r)


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE configs 3 and 4 at full depth (round 4): the reference's own 70B engine is the DYNAMIC one
# (umbrella/speculation/dynamic_speculation_engine.py:215-327, configs/greedy_config_12gb.json, chat_config_24gb.json).
T70 = "hugging-quants/Meta-Llama-3.1-70B-Instruct-AWQ-INT4"
D1B = "meta-llama/Llama-3.2-1B-Instruct"
D8BAWQ = "hugging-quants/Meta-Llama-3.1-8B-Instruct-AWQ-INT4"
LDYN = 2048
_cache = {}


def _model(name, dev, **kw):
    """one instance per (name, placement) for the whole module: a 70B-AWQ allocation is ~40 GB and ~30 s"""
    from umbrella_amd.models import AutoModelLM
    alloc_kw = {k: kw.pop(k) for k in ("num_cache_layers",) if k in kw}
    key = (name, tuple(sorted(kw.items())), tuple(sorted(alloc_kw.items())))
    if key not in _cache:
        m = AutoModelLM.from_pretrained(name, max_length=LDYN, device=str(dev), dtype=torch.float16, **kw)
        m.alloc(**alloc_kw)
        _cache[key] = m
    return _cache[key]


def _drop(pred):
    for k in [k for k in _cache if isinstance(k, tuple) and pred(k)]:
        del _cache[k]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _dyn_engine(target, draft, dev, graph, width, beams, depth, **knobs):
    from umbrella_amd.speculation.dynamic_speculation_engine import DynamicSpeculationEngine
    from umbrella_amd.speculation.speculation_utils import IdTokenizer
    e = DynamicSpeculationEngine("draft", "target", dtype=torch.float16, device=str(dev), width=width, num_beams=beams,
                                 depth=depth, max_length=LDYN, offload=False, draft_model_obj=draft, target_model_obj=target,
                                 tokenizer=IdTokenizer(), hip_graph=graph, seed=0, **knobs)
    e.initialize()
    return e


def _prompt():
    return torch.randint(3, 128000, (96,), generator=torch.Generator().manual_seed(1)).tolist()


def test_c3_resident_70b_awq_dynamic_w16_b24_d16():
    """BASELINE config 3's engine with the target resident: 80 AWQ int4 layers + 16 draft layers, dynamic tree width 16 /
    24 beams / depth 16 (T = 257: the wide verify GEMM, exact fp16 dequant), greedy.  hipGraph == eager token for token;
    every emitted token is the arg-max of the target's own T = 1 row (skinny GEMM, folded dequant) or inside the 16-bit
    near-tie band -- the two GEMM families are held together here at full depth."""
    dev = torch.device("cuda:0")
    target, draft = _model(T70, dev), _model(D1B, dev)
    prompt, new = _prompt(), 24
    eg = _dyn_engine(target, draft, dev, True, 16, 24, 16)
    out_g = eg.generate(input_ids=prompt, max_new_tokens=new)
    ee = _dyn_engine(target, draft, dev, False, 16, 24, 16)
    out_e = ee.generate(input_ids=prompt, max_new_tokens=new)
    tg, te = out_g["generated_tokens"], out_e["generated_tokens"]
    assert eg.tree_size == 257 and tg == te, "hipGraph replay and eager launches disagree"
    assert len(tg) >= new
    exact = _check_against_ar(target, prompt, tg, TOL[torch.float16], dev, "C3 resident")
    assert exact >= len(tg) - 3, (exact, len(tg))
    report_fact("full_depth/C3 resident accept", out_g["avg_accept_tokens"])


def test_c3_resident_one_int4_arithmetic_for_every_row_count():
    """VERDICT r4 missing #2: the reference runs ONE int4 kernel for every T < 1024 (awq_utils.py:67-77), so its tree verify
    and its T = 1 row share their weights' rounding.  UMB_DEQUANT=exact gives this build the same property -- the T = 1
    rows (skinny kernel) and the T = 257 verify (wide kernel) both multiply W = fp16((q - z) * s), bit for bit the
    reference's dequantised weights.  Same C3 engine as above under that switch; what is left between the two paths is
    the fp32 summation order (split-K / tile order, tree attention), and the count of exact arg-max agreements is reported
    next to the default build's."""
    dev = torch.device("cuda:0")
    os.environ["UMB_DEQUANT"] = "exact"
    try:
        target, draft = _model(T70, dev), _model(D1B, dev)
        prompt, new = _prompt(), 24
        eg = _dyn_engine(target, draft, dev, True, 16, 24, 16)
        tg = eg.generate(input_ids=prompt, max_new_tokens=new)["generated_tokens"]
        assert len(tg) >= new
        exact = _check_against_ar(target, prompt, tg, TOL[torch.float16], dev, "C3 resident, exact dequant at every row count")
        assert exact >= len(tg) - 3, (exact, len(tg))
    finally:
        os.environ.pop("UMB_DEQUANT", None)


def _penalised(row, history, penalty):
    """HF repetition penalty on the history tokens (speculation_utils.py:340-345), fp32"""
    row = row.clone()
    idx = torch.tensor(sorted(set(history)), device=row.device)
    v = row[idx]
    row[idx] = torch.where(v < 0, v * penalty, v / penalty)
    return row


def test_c4_70b_awq_with_8b_awq_draft_w32_b32_d24_stochastic():
    """BASELINE config 4: 70B-AWQ target + 8B-AWQ draft (32 int4 layers), dynamic width 32 / 32 beams / depth 24
    (T = 769), stochastic verification (temperature 0.6, top-p 0.9, top-k 32, repetition penalty 1.05).  One seed:
    hipGraph == eager draw for draw; every sampled token lies inside the top-k support of the target's own
    penalised T = 1 row (teacher forced), within the 16-bit band at the k-th logit."""
    dev = torch.device("cuda:0")
    target, draft = _model(T70, dev), _model(D8BAWQ, dev)
    knobs = dict(temperature=0.6, topp=0.9, topk=32, repetition_penalty=1.05)
    prompt, new = _prompt(), 12
    eg = _dyn_engine(target, draft, dev, True, 32, 32, 24, **knobs)
    out_g = eg.generate(input_ids=prompt, max_new_tokens=new)
    ee = _dyn_engine(target, draft, dev, False, 32, 32, 24, **knobs)
    out_e = ee.generate(input_ids=prompt, max_new_tokens=new)
    tg, te = out_g["generated_tokens"], out_e["generated_tokens"]
    assert eg.tree_size == 769 and tg == te, "hipGraph replay and eager launches disagree under one seed"
    assert len(tg) >= new
    tol = TOL[torch.float16]
    target.clear()
    row = target.prefill_tokens(torch.tensor(prompt, dtype=torch.int32, device=dev), 0)
    # token 0 is the plain arg-max of the prompt's last row with EOS masked (dynamic:130); the rest are sampled
    r0 = row.clone()
    r0[list(target.eos_tokens)] = -float("inf")
    assert float(r0.max() - r0[tg[0]]) < 2 * tol
    for i in range(1, len(tg)):
        row = target.prefill_tokens(torch.tensor([tg[i - 1]], dtype=torch.int32, device=dev), len(prompt) + i - 1)
        pen = _penalised(row, prompt + tg[:i], 1.05)
        kth = float(pen.topk(32).values[-1])
        assert float(pen[tg[i]]) >= kth - 2 * tol, f"token {i} = {tg[i]} is outside the top-32 support of its row"
    target.clear()
    report_fact("full_depth/C4 stochastic", dict(n=len(tg), accept=out_g["avg_accept_tokens"]))
    _drop(lambda k: k[0] == D8BAWQ)


@pytest.mark.parametrize("ncl", [0, 40])
def test_c3_offloaded_equals_resident(ncl):
    """BASELINE config 3 proper: the 70B-AWQ target's layers streamed from pinned host DRAM (all 80, and 40 behind a
    40-layer resident prefix with the 8-slab device ring), 1B draft, dynamic w16/b24/d16, greedy: the tokens, the accept
    lengths and the bonus tokens of every iteration equal the resident target's, token for token."""
    dev = torch.device("cuda:0")
    prompt, iters = _prompt(), 4

    def run(target):
        eng = _dyn_engine(target, _model(D1B, dev), dev, True, 16, 24, 16)
        assert eng._prefill(torch.tensor([prompt]))
        start, trace = eng.num_nodes, []
        for _ in range(iters):
            eng.step()
            trace.append((eng.num_nodes, eng.last_accept, eng.last_bonus))
        out = (trace, eng.tokens[start:eng.num_nodes + 1].tolist())
        eng.reset()
        return out

    if "resident_trace" not in _cache:
        _cache["resident_trace"] = run(_model(T70, dev))
    _drop(lambda k: k[0] == T70)                                # the resident copy makes room for the slab ring
    target = _model(T70, dev, offload=True, num_cache_layers=ncl)
    assert sum(1 for h in target.host_slabs if h is not None) == 80 - ncl
    assert target.n_slabs == (2 if ncl == 0 else 8)
    got = run(target)
    _drop(lambda k: k[0] == T70)                                # releases the pinned host slabs as well
    assert got == _cache["resident_trace"]


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE config 5 at its own workload (round 6): Llama-3.3-70B-AWQ layer-sharded over EIGHT stages, 10 layers each,
# the 1B draft on stage 0, static 3x4, greedy (umbrella_amd/parallel.py build_pipelined_engine).  A test box
# has one GPU, so the eight stage processes share it and the seven hops per forward travel through pinned host buffers
# over gloo; kernels, their order and the per-stage hipGraphs are those of an 8-GPU run -- only the transport differs.
C5_NEW = 40


def _c5_worker(rank, world, port, q, prompt, steer):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), UMBRELLA_SYNTHETIC="1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import __graft_entry__ as ge
    ge.build()
    from umbrella_amd.parallel import build_pipelined_engine, shutdown_pipeline
    from umbrella_amd.sequoia_utils import DEFAULT_ACC, generate_sequoia_tree
    from umbrella_amd.speculation.speculation_utils import IdTokenizer
    eng = build_pipelined_engine("cuda:0", dtype=torch.float16, engine="static", model=T70, draft_model=D1B,
                                 growmap=generate_sequoia_tree(3, 4), max_length=512, exit_layer=16, safe_buffer=16,
                                 tokenizer=IdTokenizer())
    if eng is not None:
        raw = eng.generate(input_ids=prompt, max_new_tokens=C5_NEW)
        # steered draft: the single-process engine's fixed-point continuation placed in the tree (bench.py's knob)
        assert eng._prefill(torch.tensor([prompt]))
        start = eng.num_nodes
        eng.set_oracle_draft(steer, start, DEFAULT_ACC, seed=0)
        steps = 0
        while eng.num_nodes - start < C5_NEW and eng.validate_status():
            eng.step()
            steps += 1
        torch.cuda.synchronize()
        tk = eng.tokens[start:start + C5_NEW + 1].tolist()
        accept = (eng.num_nodes - start) / max(steps, 1)
        hop_bytes = eng.tree_size * eng._stage_model.config.hidden_size * 2
        eng.reset()
        shutdown_pipeline(eng)
        q.put(dict(raw=raw["generated_tokens"], raw_accept=raw["avg_accept_tokens"], steered=tk, accept=accept,
                   diverged=eng.diverged, layers_per_rank=eng._stage_model.num_layers, hop_bytes=hop_bytes,
                   tree_size=eng.tree_size))
    dist.barrier()
    dist.destroy_process_group()


def test_c5_70b_awq_eight_stages():
    """BASELINE config 5: eight processes x 10 of the 70B-AWQ's 80 layers (4.5 GB of int4 each), draft = all 16 layers of
    the 1B on stage 0, Sequoia 3x4 (T = 13: 13 x 8192 x 2 B = 213 KB per hop).  Token ids == the single-process headline
    engine's (default schedules, persistent draft chain included) for >= 40 tokens with the raw random draft, and with
    the steered one up to a committed, margin-checked near-tie, where either side of the tie is accepted."""
    import socket
    import torch.multiprocessing as mp
    import __graft_entry__ as ge
    ge.build()
    from umbrella_amd.sequoia_utils import DEFAULT_ACC, generate_sequoia_tree
    from umbrella_amd.speculation.speculation_utils import IdTokenizer
    from umbrella_amd.speculation.static_speculation_engine import StaticSpeculationEngine
    dev = torch.device("cuda:0")
    _drop(lambda k: True)                                             # the module's cached 70B / drafts: eight stages need the room
    prompt = _prompt()
    ref = StaticSpeculationEngine(D1B, T70, dtype=torch.float16, device=str(dev), growmap=generate_sequoia_tree(3, 4),
                                  max_length=512, exit_layer=16, safe_buffer=16, tokenizer=IdTokenizer())
    ref.initialize()
    raw = ref.generate(input_ids=prompt, max_new_tokens=C5_NEW)
    truth = _ar(ref.target_model, prompt, C5_NEW + 16, dev)
    for _ in range(8):                                                # fixed point of the steered run, as in _run_pair
        assert ref._prefill(torch.tensor([prompt]))
        start = ref.num_nodes
        ref.set_oracle_draft(truth, start, DEFAULT_ACC, seed=0)
        steps = 0
        while ref.num_nodes - start < C5_NEW and ref.validate_status():
            ref.step()
            steps += 1
        accept, div = (ref.num_nodes - start) / max(steps, 1), ref.diverged
        while ref.num_nodes - start < C5_NEW + 16 and ref.validate_status():
            ref.step()
        tk = ref.tokens[start:start + C5_NEW + 1].tolist()
        steer = truth
        truth = ref.tokens[start:ref.num_nodes + 1].tolist()
        ref.reset()
        if div == 0:
            break
    assert div == 0
    del ref
    torch.cuda.synchronize()
    torch.cuda.empty_cache()

    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_c5_worker, args=(r, 8, port, q, prompt, steer)) for r in range(8)]
    for p in procs:
        p.start()
    try:
        got = q.get(timeout=900)
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert got["layers_per_rank"] == 10 and got["tree_size"] == 13 and got["hop_bytes"] == 13 * 8192 * 2
    assert len(got["raw"]) >= C5_NEW and got["raw"] == raw["generated_tokens"]
    # The single-process steered run is the headline pair's (same models, tree and prompt).  Where the committed near-tie list
    # records a margin-checked 16-bit near-tie of that run, the eight stages may take the other side of it: token for token up
    # to that position, there one of the tie's two candidates; after it the two continuations have different contexts.
    ties = {m[0]: (m[1], m[2]) for m in _TIES.get("headline 70B-AWQ + 1B 3x4/steered draft", [])}
    switch = next((i for i, (a, b) in enumerate(zip(got["steered"], tk)) if a != b), None)
    assert len(got["steered"]) == len(tk) and accept > 2.0
    if switch is None:
        assert got["diverged"] == 0 and abs(got["accept"] - accept) < 1e-9
    else:
        assert switch in ties and got["steered"][switch] in ties[switch], (switch, got["steered"][switch], tk[switch], ties)
    report_fact("full_depth/C5 70B-AWQ x 8 stages", dict(layers_per_rank=got["layers_per_rank"], hop_bytes=got["hop_bytes"],
                tokens_raw=len(got["raw"]), tokens_steered=len(got["steered"]), accept_steered=got["accept"],
                raw_accept=got["raw_accept"], equals_single_process=switch is None, near_tie_taken_otherwise_at=switch))
