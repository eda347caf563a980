"""FP8 (OCP e4m3fn) weight-only linears on the GPU: umb_fp8_repack + format 2 of umb_gemm / umb_gemm_fused, bit for bit
against the float64 restatement of tests/fp8_ref.py, then Llama / Qwen3 models loaded from FP8 Hugging Face directories in
both naming schemes, both engines, and two 70B-wide layers.

umb_gemv, the persistent chain and umb_head_stream take plain 16-bit rows and carry no weight-format argument, so there is
no format-2 call to refuse there; the model forwards refuse FP8 layers in a GEMV / chain / fused workspace (checked below)."""
import copy
import ctypes as C
import json
import os

import pytest
import torch

import fp8_ref as fr
from hip_helpers import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
EINVAL = -22
# the project's criterion for a dense model's logits against an fp32 restatement (tests/test_qwen3.py, test_gemma2.py):
# |got - ref| <= TOL[dtype] * max(1, max|ref| / 16) + max|ref| * (one rounding of the logits to the dtype)
REL = {torch.float16: 2.0 ** -9, torch.bfloat16: 2.0 ** -6}
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "growmaps.json")) as f:
    GM = json.load(f)


def _fact(name, value):
    from conftest import report_fact
    report_fact(name, value)


def _pack(codes, rows, mode=0, D=0, rope_heads=0):
    from umbrella_amd.models.llama import PackedLinear
    return PackedLinear.from_fp8(codes.to(DEV), rows.to(DEV), interleave=(mode == 1), rope=(D, rope_heads) if mode == 2 else None)


def _gemm(lin, x, S, R=1, epi=0, fm=False, rc_only=False):
    """format-2 launch -> fp32 partials [S][T][N] (epi 0 / 1) prefilled with NaN, or the 16-bit act [T][N/2] (epi 2)"""
    from umbrella_amd import _lib
    from umbrella_amd.models.llama import to_fm
    T = x.shape[0]
    if epi == 2:
        out = torch.zeros(T, lin.N // 2, dtype=x.dtype, device=DEV)
    else:
        out = torch.full((S, T, lin.N), float("nan"), dtype=torch.float32, device=DEV)
    fx = _lib.UmbGemmFused()
    xin, ldx = x, x.stride(0)
    if fm:
        xin, ldx = to_fm(x.contiguous()), lin.K
        fx.pad1 = 1
    rc = _lib.load().umb_gemm_fused(_lib.ptr(out), _lib.ptr(xin), ldx, _lib.ptr(lin.w), _lib.ptr(lin.meta), T, lin.N, lin.K, 2, S,
                                    R, epi, C.byref(fx), _lib.dtype_code(x.dtype), _lib.stream_ptr())
    torch.cuda.synchronize()
    if rc_only:
        return rc
    assert rc == 0, rc
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_every_code_reads_back(dtype, mode):
    """one-hot activation rows x = e_k against a 64 x 256 matrix holding all 254 finite codes in every row (+-0 and the
    subnormals included) under arbitrary real fp32 scales: out[k][n] == fl32(scale[n'][k / 128] * value(w8[n'][k])) bit for
    bit, n' the source row of packed row n -- the row maps and the metadata permutation are read back too.  (A zero sum is
    +0: the accumulator starts there.)"""
    N, K, D, RH = 64, 256, 16, 3
    codes_all = fr.finite_codes()
    n_i, k_i = torch.meshgrid(torch.arange(N), torch.arange(K), indexing="ij")
    codes = codes_all[(k_i + 7 * n_i) % 254]
    assert all(len(set(codes[n].tolist())) == 254 for n in range(N))
    rows = torch.rand(N, K // 128, generator=torch.Generator().manual_seed(mode)) * 3.0 + 0.01
    lin = _pack(codes, rows, mode, D, RH)
    x = torch.eye(K, dtype=dtype, device=DEV)                         # 256 rows: four 64-row launches
    got = _gemm(lin, x, 1)[0].cpu()
    src = torch.tensor([fr.rowmap(n, N, mode, D, RH) for n in range(N)])
    val = fr.code_values(codes).float()[src]                          # [N][K] in packed row order
    want = (rows[src].repeat_interleave(128, dim=1) * val).t().contiguous() + 0.0
    assert torch.equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())


_SHAPES_T = (1, 3, 13, 16, 17, 32, 33, 64, 65, 129)
_REF = {}


def _operands(N, K, dtype):
    """(codes, rows, x [129][K], {S: float64 partials [S][129][N]}) -- computed once per (N, K, dtype), never modified"""
    key = (N, K, dtype)
    if key not in _REF:
        codes, rows, x = fr.int_operands(N, K, 129, seed=N * 7 + K, dtype=dtype)
        refs = {S: fr.gemm_ref(codes, rows, x, S) for S in (1, 2, 3, 5)}
        for r in refs.values():
            assert torch.equal(r.float().double(), r)                 # exactly representable: any fp32 order gives it
        _REF[key] = (codes, rows, x, refs)
    return _REF[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [64, 192, 1024])
def test_every_slab_bit_for_bit(dtype, N):
    """integer codes |w| <= 8, integer activations, power-of-two scales: every split slab of every launch equals the float64
    restatement bit for bit.  T x K x S in full for one n-tile per wave; ragged and empty trailing slabs (K / 128 = 3, S = 5)
    in NaN-prefilled buffers; then ldx > K, FM-ordered activations, R = 2 and the plan's tb word (4-wave and 8-wave blocks)."""
    n = 0
    for K in (128, 384, 1024):
        codes, rows, x, refs = _operands(N, K, dtype)
        lin = _pack(codes, rows)
        xd = x.to(DEV)
        wide = torch.zeros(129, K + 64, dtype=dtype, device=DEV)
        wide[:, :K] = xd
        for T in _SHAPES_T:
            for S in (1, 2, 3, 5):
                want = refs[S][:, :T].float()
                got = _gemm(lin, xd[:T], S).cpu()
                assert torch.equal(_bits(got), _bits(want + 0.0)), (T, K, S)
                n += 1
                if T in (13, 33, 64, 129) and S in (1, 3):
                    variants = [dict(R=1 | (3 << 8)), dict(R=1 | ((6 | 0x80) << 8)), dict(R=2), dict(R=2 | (7 << 8))]
                    for kw in variants:
                        assert torch.equal(_bits(_gemm(lin, xd[:T], S, **kw).cpu()), _bits(want + 0.0)), (T, K, S, kw)
                    assert torch.equal(_bits(_gemm(lin, wide[:T, :K], S).cpu()), _bits(want + 0.0)), (T, K, S, "ldx")
                    if T <= 64:
                        assert torch.equal(_bits(_gemm(lin, xd[:T], S, fm=True).cpu()), _bits(want + 0.0)), (T, K, S, "fm")
                        assert torch.equal(_bits(_gemm(lin, xd[:T], S, R=2, fm=True).cpu()), _bits(want + 0.0)), (T, K, S, "fm2")
                    n += 6
        if K == 384:
            assert bool((refs[5][3:] == 0).all())                      # the two empty slabs, written as zeros over the NaNs
    _fact(f"fp8/slab launches bit-exact N={N} {str(dtype)[6:]}", n)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batch_invariance_on_real_operands(dtype):
    """row t of a 13-row and of a 129-row launch equals the 1-row launch of that row, bit for bit, on real-valued operands
    (every finite code, Gaussian activations, real scales) and with the plan's own (R, S, tb)"""
    g = torch.Generator().manual_seed(9)
    for (N, K) in ((192, 1024), (1024, 384)):
        codes = fr.finite_codes()[torch.randint(0, 254, (N, K), generator=g)]
        rows = torch.rand(N, K // 128, generator=g) * 0.02 + 0.001
        lin = _pack(codes, rows)
        x = torch.randn(129, K, generator=g).to(dtype).to(DEV)
        for S, R in ((lin.S, lin.Rtb), (3, 1), (2, 2)):
            big, mid = _gemm(lin, x, S, R), _gemm(lin, x[:13], S, R)
            for t in (0, 5, 12, 63, 64, 128):
                one = _gemm(lin, x[t:t + 1], S, R)
                assert torch.equal(_bits(one[:, 0]), _bits(big[:, t])), (N, K, S, R, t)
                if t < 13:
                    assert torch.equal(_bits(one[:, 0]), _bits(mid[:, t])), (N, K, S, R, t)
        # and the launch is the restatement to fp32 accumulation error
        ref = fr.gemm_ref(codes, rows, x, lin.S).sum(0)
        got = _gemm(lin, x, lin.S, lin.Rtb).double().sum(0).cpu()
        bound = (x.cpu().double().abs() @ (fr.code_values(codes).abs() * rows.double().repeat_interleave(128, 1)).t()) * K * 2.0 ** -24
        assert bool(((got - ref).abs() <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T", [5, 64])
def test_silu_epilogue_row_by_row(dtype, T):
    """epi 2 on interleaved [gate; up] rows (repack mode 1): act[t][m] = rnd(rnd(silu(rnd(gate))) * rnd(up)).  Integer
    operands make gate and up exact, so what is left is the kernel's __expf (relative error far below half a unit of either
    dtype, which can move rnd(silu) by one unit) and the product's rounding: two units of the dtype, relative."""
    N, K = 256, 128
    codes, _, x = fr.int_operands(N, K, T, seed=T, dtype=dtype)
    rows = torch.pow(2.0, torch.randint(-7, -4, (N, 1), generator=torch.Generator().manual_seed(T)).float())
    lin = _pack(codes, rows, mode=1)
    assert lin.S == 1
    for fm in (False, True):
        got = _gemm(lin, x.to(DEV), 1, lin.Rtb, epi=2, fm=fm).float().cpu()
        acc = fr.gemm_ref(codes, rows, x, 1)[0].float()                # [T][N], source row order: [gate; up]
        gate, up = acc[:, :N // 2].to(dtype).float(), acc[:, N // 2:].to(dtype).float()
        want = (torch.nn.functional.silu(gate).to(dtype).float() * up).to(dtype).float()
        assert bool(torch.isfinite(want).all())
        err = (got - want).abs()
        tol = want.abs() * REL[dtype] + 2.0 ** -23 * (1.0 + up.abs())      # + two steps of the fp16 subnormal grid (2^-24) times |up|
        assert bool((err <= tol).all()), float((err / tol).max())
        assert float(want.abs().max()) > 1.0


def test_contract_refusals():
    """epi 3 / 4, N % 64 != 0 and umb_gemm_ll with format 2 return UMB_EINVAL (no launch: the NaN prefill stays)"""
    from umbrella_amd import _lib
    lib = _lib.load()
    codes, rows, x = fr.int_operands(64, 128, 4, seed=1)
    lin = _pack(codes, rows)
    xd = x.to(DEV)
    for epi in (3, 4):
        assert _gemm(lin, xd, 1, epi=epi, rc_only=True) == EINVAL
    out = torch.full((4, 80), float("nan"), dtype=torch.float32, device=DEV)
    st = _lib.stream_ptr()
    assert lib.umb_gemm(_lib.ptr(out), _lib.ptr(xd), 128, _lib.ptr(lin.w), _lib.ptr(lin.meta), 4, 80, 128, 2, 1, 1, 0, 0, st) == EINVAL
    assert lib.umb_gemm(_lib.ptr(out), _lib.ptr(xd), 128, _lib.ptr(lin.w), _lib.ptr(lin.meta), 4, 64, 128, 3, 1, 1, 0, 0, st) == EINVAL
    assert lib.umb_gemm(_lib.ptr(out), _lib.ptr(xd), 128, _lib.ptr(lin.w), None, 4, 64, 128, 2, 1, 1, 0, 0, st) == EINVAL
    w = torch.zeros(80 * 128, dtype=torch.uint8, device=DEV)
    assert lib.umb_fp8_repack(_lib.ptr(w), _lib.ptr(w), _lib.ptr(w), _lib.ptr(w), 80, 128, 0, 0, 0, st) == EINVAL
    assert lib.umb_fp8_repack(_lib.ptr(w), _lib.ptr(w), _lib.ptr(w), _lib.ptr(w), 64, 192, 0, 0, 0, st) == EINVAL
    fx = _lib.UmbGemmLL()
    assert lib.umb_gemm_ll(_lib.ptr(out), _lib.ptr(xd), _lib.ptr(lin.w), _lib.ptr(lin.meta), 4, 64, 128, 2, 0, C.byref(fx), 0, st) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the plan of format 2: one byte per weight, the dense rule with >= 512 k per slab
    R, S = C.c_int(0), C.c_int(0)
    lib.umb_gemm_plan(8192, 8192, 2, 0, C.byref(R), C.byref(S))
    assert (R.value, S.value) == (1, 8)
    lib.umb_gemm_plan(8192, 1024, 2, 0, C.byref(R), C.byref(S))
    assert (R.value, S.value) == (1, 2)


# ----------------------------------------------------------------------------- models
def _load(path, dtype, max_length=256, **kw):
    from umbrella_amd.models.auto_model import AutoModelLM
    m = AutoModelLM.from_pretrained(path, dtype=dtype, max_length=max_length, device=DEV, **kw)
    m.alloc()
    return m


def _oracle_logits(path, kind, dense, ids):
    """fp32 torch oracle over a causal prompt, given the dequantised (w8.float() * scale) weights"""
    if kind.startswith("qwen3"):
        import qwen3_ref as qr
        return qr.Qwen3Ref(dict(fr.TINY[kind]), dense).forward(ids)
    from oracle import ops as O
    from oracle.model import OracleLlama
    from umbrella_amd.models.config import LlamaCfg
    cfg = LlamaCfg.from_dir(path)
    inv, scale = O.rope_inv_freq(cfg.head_dim, cfg.rope_theta, cfg.rope_scaling)
    n = len(ids)
    o = OracleLlama(cfg, dense, inv, scale, max_length=n + 1, dtype=torch.float32)
    return o.inference(torch.tensor([ids]), torch.arange(n)[None], torch.tril(torch.ones(n, n + 1, dtype=torch.bool)),
                       torch.arange(n))[0]


def _prompt_logits(m, ids):
    n = len(ids)
    mask = torch.tril(torch.ones(n, m.max_length, dtype=torch.bool))
    return m.inference(torch.tensor([ids]), torch.arange(n)[None], mask, torch.arange(n))[0].cpu()


def _bound(ref, dtype):
    top = float(ref.abs().max())
    return TOL[dtype] * max(1.0, top / 16.0) + top * REL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind,scheme", [("llama256", "channel"), ("llama256", "tensor"), ("llama2048", "block128"),
                                         ("qwen2", "block128"), ("qwen3", "block128"), ("qwen3", "channel"),
                                         ("qwen3_2048", "block128")])
def test_models_from_fp8_directories(tmp_path, dtype, kind, scheme):
    """tiny Llama (H 256: in-place norm layer; H 2048: the deferred-norm layer, which csrc/model.hip takes at H % 2048 == 0;
    Qwen2-style bias) and Qwen3, loaded from FP8 directories in both naming schemes, against the fp32 oracle on
    w8.float() * scale weights, at 20 rows (row-major operands) and 40 rows (FM operands)"""
    path = str(tmp_path)
    _, dense = fr.write_fp8_dir(path, kind, scheme, dtype=dtype)
    m = _load(path, dtype)
    assert m.config.fp8 and m.sched == "split" and m._ws.fused == 0
    assert all(ln.awq == 2 for lins in m.layers for ln in lins.values()) and m.lm_head.awq == 0
    ids = torch.randint(6, 512, (40,), generator=torch.Generator().manual_seed(3)).tolist()
    ref = _oracle_logits(path, kind, dense, ids)
    worst = 0.0
    for n in (20, 40):
        m.clear()
        got = _prompt_logits(m, ids[:n])
        err = float((got - ref[:n]).abs().max())
        worst = max(worst, err)
        assert err <= _bound(ref[:n], dtype), (n, err, _bound(ref[:n], dtype))
    _fact(f"fp8/model {kind} {scheme} {str(dtype)[6:]} worst |logit gap|", {"gap": round(worst, 5), "bound": round(_bound(ref, dtype), 5),
                                                                            "max|ref|": round(float(ref.abs().max()), 3)})
    # FP8 layers in a workspace of another schedule are refused by the native forward
    from umbrella_amd._lib import UmbError
    m._ws.fused = 2
    with pytest.raises(UmbError):
        _prompt_logits(m, ids[:4])
    m._ws.fused = 0


@pytest.mark.parametrize("rows", [5, 20])
@pytest.mark.parametrize("kind,scheme", [("llama256", "channel"), ("llama2048", "block128"), ("qwen3", "block128"),
                                         ("qwen3_2048", "channel")])
def test_graph_equals_eager_bit_for_bit(tmp_path, kind, scheme, rows):
    """an FP8 Llama and an FP8 Qwen3 loaded from the directories with cuda_graph=True, on the in-place (H 256) and the
    deferred-norm (H 2048) layer, at 5 rows (row-major operands) and 20 rows (FM operands): forward_explicit captured into a
    graph and replayed leaves the same logits, bit for bit, as the eager call (pattern of test_qwen3_graph_equals_eager)"""
    dtype = torch.bfloat16
    path = str(tmp_path)
    fr.write_fp8_dir(path, kind, scheme, dtype=dtype)
    m = _load(path, dtype, cuda_graph=True)
    assert m.config.fp8 and m._ws.fused == 0
    dev = torch.device(DEV)
    T = rows
    ids = torch.randint(6, 512, (T,), generator=torch.Generator().manual_seed(4)).to(dtype=torch.int32, device=dev)
    pos = torch.arange(T, dtype=torch.int32, device=dev)
    pre = torch.zeros(1, dtype=torch.int32, device=dev)
    m.forward_explicit(ids, pos, pos, pre, head_from=0)
    eager = m.logits_buffer[:T].clone()
    assert bool(torch.isfinite(eager).all()) and float(eager.abs().max()) > 1.0
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m.forward_explicit(ids, pos, pos, pre, head_from=0)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.forward_explicit(ids, pos, pos, pre, head_from=0)
    m.logits_buffer.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(m.logits_buffer[:T], eager)


@pytest.mark.parametrize("kind,scheme", [("llama256", "channel"), ("qwen3", "block128")])
def test_prompt_chunks_of_65_and_129_rows(tmp_path, kind, scheme):
    """a prompt fed as one 65- / 129-row forward (64-row launches of the same kernel inside) against the same prompt fed in
    <= 64-row forwards: last-row logits within the model tolerance, both within it of the oracle"""
    dtype = torch.float16
    path = str(tmp_path)
    _, dense = fr.write_fp8_dir(path, kind, scheme, dtype=dtype)
    ids = torch.randint(6, 512, (129,), generator=torch.Generator().manual_seed(5)).tolist()
    small, big = _load(path, dtype), _load(path, dtype)
    big.reserve(144, logit_rows=64)
    assert small.ws_tokens == 64 and big.ws_tokens >= 129
    for n in (65, 129):
        ref = _oracle_logits(path, kind, dense, ids[:n])[-1]
        t = torch.tensor(ids[:n], dtype=torch.int32, device=DEV)
        small.clear(); big.clear()
        a = small.prefill_tokens(t, 0).float().cpu().clone()
        b = big.prefill_tokens(t, 0).float().cpu().clone()
        bound = _bound(ref, dtype)
        gap = float((a - b).abs().max())
        assert gap <= bound and float((a - ref).abs().max()) <= bound and float((b - ref).abs().max()) <= bound
        _fact(f"fp8/prompt chunk {n} rows vs <= 64-row feed {kind}", {"gap": round(gap, 5), "bound": round(bound, 5)})


def _engine(path_t, path_d, engine, dtype, hip_graph=True, **kw):
    from umbrella_amd.speculation.dynamic_speculation_engine import DynamicSpeculationEngine
    from umbrella_amd.speculation.speculation_utils import IdTokenizer
    from umbrella_amd.speculation.static_speculation_engine import StaticSpeculationEngine
    target = _load(path_t, dtype)
    draft = _load(path_d, dtype, cuda_graph=(engine == "static"))
    common = dict(dtype=dtype, device=DEV, max_length=256, safe_buffer=16, stop_distance=8, draft_model_obj=draft,
                  target_model_obj=target, tokenizer=IdTokenizer(), hip_graph=hip_graph, **kw)
    if engine == "static":
        eng = StaticSpeculationEngine("d", "t", growmap=GM["3x4"], **common)
    else:
        eng = DynamicSpeculationEngine("d", "t", width=8, num_beams=8, depth=4, **common)
    eng.initialize()
    return eng


@pytest.mark.parametrize("engine", ["static", "dynamic"])
def test_engines_with_fp8_target_and_fp8_draft(tmp_path, engine):
    """static 3x4 and dynamic (width 8, depth 4) greedy, FP8 target (per-channel scales) and FP8 draft (another model, block
    scales), loaded from directories with no environment knob: every emitted token is an arg-max of the target's own eager
    run over the sequence within the 16-bit near-tie slack of tests/hip_helpers.py; hipGraph == eager, token for token"""
    dtype = torch.float16
    pt, pd = str(tmp_path / "t"), str(tmp_path / "d")
    fr.write_fp8_dir(pt, "llama256", "channel", dtype=dtype)
    fr.write_fp8_dir(pd, "llama256", "block128", seed=12, dtype=dtype)
    prompt = torch.randint(6, 512, (24,), generator=torch.Generator().manual_seed(8)).tolist()
    outs = []
    for graph in (True, False):
        eng = _engine(pt, pd, engine, dtype, hip_graph=graph)
        assert eng.target_model.config.fp8 and eng.draft_model.config.fp8 and not getattr(eng.draft_model, "gemv", False)
        outs.append(eng.generate(input_ids=prompt, max_new_tokens=32))
        target = eng.target_model
    toks = outs[0]["generated_tokens"]
    assert toks == outs[1]["generated_tokens"] and len(toks) >= 8
    seq = prompt + toks
    target.clear()
    logits = _prompt_logits(target, seq[:64])
    worst = 0.0
    for i, tok in enumerate(toks[:64 - len(prompt)]):
        row = logits[len(prompt) + i - 1].clone()
        if i == 0 and engine == "dynamic":
            row[[3, 5]] = -float("inf")
        worst = max(worst, float(row.max() - row[tok]))
        assert float(row.max() - row[tok]) <= TOL[dtype], (i, tok, float(row.max() - row[tok]))
    _fact(f"fp8/engine {engine} greedy", {"tokens": len(toks), "accept": round(outs[0]["avg_accept_tokens"], 3),
                                          "worst_gap_to_own_argmax": round(worst, 5)})


def test_static_engine_stochastic_reference_sampler(tmp_path):
    """one stochastic case (reference_sampler=True) with an FP8 target and draft: runs to length, hipGraph == eager"""
    dtype = torch.float16
    pt = str(tmp_path / "t")
    fr.write_fp8_dir(pt, "llama256", "tensor", dtype=dtype)
    prompt = torch.randint(6, 512, (24,), generator=torch.Generator().manual_seed(8)).tolist()
    outs = []
    for graph in (True, False):
        eng = _engine(pt, pt, "static", dtype, hip_graph=graph, reference_sampler=True, temperature=0.7, topp=0.9, topk=16,
                      repetition_penalty=1.1, seed=11)
        outs.append(eng.generate(input_ids=prompt, max_new_tokens=24)["generated_tokens"])
    assert outs[0] == outs[1] and len(outs[0]) >= 8 and all(0 <= t < 512 for t in outs[0])


def test_full_width_70b_fp8_layers_vs_fp32():
    """Llama-3.1-70B dims (H 8192, I 28672, 64 / 8 heads, D 128, V 128256), two layers of synthetic FP8 weights with
    128 x 128 block scales: a 64-token causal prefix + a 13-node Sequoia tree against an fp32 restatement built from the
    oracle's ops on w8.float() * scale (pattern and criterion of test_full_width_70b_awq_layers_vs_fp32)."""
    import torch.nn.functional as F
    from oracle import ops as O
    from umbrella_amd.models import fp8_format
    from umbrella_amd.models.config import KNOWN, rope_inv_freq
    from umbrella_amd.models.llama import Llama
    from umbrella_amd.models.synthetic import linear_shapes, synth_fp8_tensors
    dev = torch.device(DEV)
    name, dtype = next(k for k, c in KNOWN.items() if c.fp8 and c.hidden_size == 8192), torch.float16
    cfg = copy.copy(KNOWN[name])
    cfg.num_hidden_layers, cfg.fp8_scheme = 2, "block128"
    gen = torch.Generator(device=dev).manual_seed(3)
    H, V = cfg.hidden_size, cfg.vocab_size
    sd = {"model.embed_tokens.weight": (torch.randn(V, H, device=dev, generator=gen) * 0.05).to(dtype),
          "lm_head.weight": (torch.randn(V, H, device=dev, generator=gen) * 0.02).to(dtype),
          "model.norm.weight": (1 + 0.1 * torch.randn(H, device=dev, generator=gen)).to(dtype)}
    dense = {}
    for i in range(2):
        p = f"model.layers.{i}."
        for ln, (n, k) in linear_shapes(cfg).items():
            w8, sc = synth_fp8_tensors(n, k, "block128", dev, gen, 0.02)
            sd[p + ln + ".weight"], sd[p + ln + ".weight_scale_inv"] = w8, sc
            dense[p + ln] = (w8.view(torch.uint8), fp8_format.expand_scale(sc, n, k))
        for nm in ("input_layernorm", "post_attention_layernorm"):
            sd[p + nm + ".weight"] = (1 + 0.1 * torch.randn(H, device=dev, generator=gen)).to(dtype)
    m = Llama(name, max_length=256, device=DEV, dtype=dtype, state_dict=sd, config=cfg)
    m.alloc()
    m.reserve(96)
    gm = GM["3x4"]
    P, T = 64, gm["size"]
    n = P + T
    ids = torch.randint(3, 128000, (1, n), generator=torch.Generator().manual_seed(5))
    pos = torch.cat([torch.arange(P), P + torch.tensor(gm["depth"])])
    mask = torch.zeros(n, n, dtype=torch.bool)
    mask[:P, :P] = torch.tril(torch.ones(P, P, dtype=torch.bool))
    mask[P:, :P] = True
    mask[P:, P:] = torch.tensor(gm["mask"]) == 1
    got = m.inference(ids, pos[None], mask, torch.arange(n))[0]
    inv, scl = rope_inv_freq(cfg)
    cos, sin = (t.to(dev) for t in O.rope_cache(inv, scl, 256, dtype))
    lin = lambda x, base: x @ fp8_format.dequant(*dense[base]).t()      # noqa: E731
    h = F.embedding(ids[0].to(dev), sd["model.embed_tokens.weight"]).float()
    md, pd = mask.to(dev), pos.to(dev)
    for i in range(2):
        p = f"model.layers.{i}."
        x = O.rmsnorm(h, sd[p + "input_layernorm.weight"].float(), cfg.rms_norm_eps)
        q = lin(x, p + "self_attn.q_proj").view(n, 64, 128)
        k = lin(x, p + "self_attn.k_proj").view(n, 8, 128)
        v = lin(x, p + "self_attn.v_proj").view(n, 8, 128)
        q, k = O.apply_rope(q, k, cos.float(), sin.float(), pd)
        a = O.masked_attention(q, k, v, md).reshape(n, 8192)
        h = h + lin(a, p + "self_attn.o_proj")
        x = O.rmsnorm(h, sd[p + "post_attention_layernorm.weight"].float(), cfg.rms_norm_eps)
        h = h + lin(F.silu(lin(x, p + "mlp.gate_proj")) * lin(x, p + "mlp.up_proj"), p + "mlp.down_proj")
    ref = O.rmsnorm(h, sd["model.norm.weight"].float(), cfg.rms_norm_eps) @ sd["lm_head.weight"].float().t()
    err = (got - ref).abs()
    scale = max(1.0, float(ref.abs().max()) / 16.0)
    bound = 0.06 * scale + float(ref.abs().max()) * 2.0 ** -9
    _fact("fp8/full width 70B two layers vs fp32", {"gap": round(float(err.max()), 5), "bound": round(bound, 5)})
    assert float(err.max()) <= bound, (float(err.max()), float(ref.abs().max()))
    top2 = ref[P:].topk(2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 4 * float(err.max())
    assert torch.equal(got[P:].argmax(-1)[clear], ref[P:].argmax(-1)[clear])
