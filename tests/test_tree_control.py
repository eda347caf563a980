"""Tree control (umbrella_amd/csrc/sample.hip): which nodes were accepted, which children were grown, which KV rows were
kept -- exactly, at the tree sizes the engines run (T = 257 / 505 / 769, up to the kernels' limit of 1024).

Every buffer a kernel is handed is pre-filled with sentinels and compared WHOLE with the expectation, so a store outside
the documented range fails.  The references are plain numpy / torch on the CPU, written from the reference project's
lines and not from the kernels' formulation:

* accept scan: the mask-sum form of dynamic_speculation_engine.py:283-309 (`ref_accept`), not the kernel's parent walk.
* beam expand: dynamic:236-248 in float64 (`ref_beam`), ordered (score descending, flat index ascending).
* KV compaction: slot n_old + i <- old slot n_old + path[i], all read before any is written (umbrella/attn/cache.py:41-49),
  on caches whose 16-bit elements are codes that name (key, feature): a misplaced element is named, not averaged away.
* arg-max / top-k: a stable descending sort (value descending, index ascending; -0.0 == +0.0) -- the rule the header
  documents and torch.argmax follows (torch.topk leaves the order of ties unspecified, so it is not the reference).

Score tolerance of the beam tests (the only tolerance in this file): MEASURED at run time as the largest difference
between the float64 reference and the same formula in fp32 torch over the test's own inputs, times 4 for expf / logf
implementation differences, capped for a single level by the 1e-5 of test_beam_expand_matches_reference_trace.
Measured here: 1.3e-6 over the single-level inputs (bound 5.1e-6); accumulated over the chained trees 1.2e-6 at
w16 b24 d16 (bound 4.8e-6) and 2.6e-6 at w32 b32 d24 (bound 1.05e-5).

The CPU tests (no gpu mark) check the builders and references against brute force, establish the tolerance and the 2 % cap
on "membership only" children, and run models of the kernels with one deliberate defect each through the same assertions
the GPU tests use: each defect must be caught.  The gpu mark is set per test, not by a module-level pytestmark.
"""
import glob
import json
import os
from collections import defaultdict

import numpy as np
import pytest
import torch

from umbrella_amd.attn.cache import VT_PAD, k_offsets, k_to_frag, vt_offsets, vt_to_frag
from umbrella_amd.models.llama import pack_mask_bits

gpu = pytest.mark.gpu
SENT = -777
BASE, ALPHA, NOMATCH = 10, 5, 7          # drafted tokens come from {BASE .. BASE + ALPHA - 1}; NOMATCH matches no drafted token
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from umbrella_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _i32(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(dev)


# ============================================================================= 1. tree builders
class Tree:
    """parents int32 [T] (topological: parents[i] < i, parents[0] = 0), depth [T], mask bool [T, T] (row i = i and its
    ancestors), bits int64 [T, ceil(T / 64)]"""

    def __init__(self, parents):
        self.parents = np.asarray(parents, dtype=np.int32)
        T = self.T = len(self.parents)
        self.depth = np.zeros(T, dtype=np.int32)
        self.mask = np.zeros((T, T), dtype=bool)
        self.mask[0, 0] = True
        for i in range(1, T):
            p = int(self.parents[i])
            assert 0 <= p < i
            self.depth[i] = self.depth[p] + 1
            self.mask[i] = self.mask[p]
            self.mask[i, i] = True
        self.bits = pack_mask_bits(torch.from_numpy(self.mask))

    def chain(self, v):
        out = [int(v)]
        while out[-1] != 0:
            out.append(int(self.parents[out[-1]]))
        return out[::-1]


def level_tree(W, depth, rs):
    """the dynamic engine's shape: root, then `depth` levels of W nodes whose parents lie in the previous level"""
    parents, prev = [0], [0]
    for lv in range(depth):
        parents += sorted(int(p) for p in rs.choice(prev, size=W))
        prev = list(range(1 + lv * W, 1 + (lv + 1) * W))
    return Tree(parents)


def random_tree(T, rs, kind="random"):
    if kind == "chain":
        return Tree([0] + list(range(T - 1)))
    if kind == "star":
        return Tree([0] * T)
    return Tree([0] + [int(rs.randint(0, i)) for i in range(1, T)])


def draft_tokens(parents, rs):
    """siblings distinct (what a top-k gives), cousins collide often (ALPHA tokens per sibling group)"""
    T = len(parents)
    tok = np.zeros(T, dtype=np.int32)
    tok[0] = BASE + rs.randint(ALPHA)
    kids = defaultdict(list)
    for c in range(1, T):
        kids[int(parents[c])].append(c)
    for cs in kids.values():
        tok[cs] = BASE + rs.permutation(max(ALPHA, len(cs)))[:len(cs)]
    return tok


ACCEPT_T = [1, 2, 13, 63, 64, 65, 128, 129, 257, 505, 769, 1023, 1024]
LEVEL = {257: (16, 16), 505: (21, 24), 769: (32, 24)}


def accept_trees(T):
    rs = np.random.RandomState(1000 + T)
    if T in LEVEL:
        return [("level", level_tree(*LEVEL[T], rs))]
    if T <= 2:
        return [("chain", random_tree(T, rs, "chain"))]
    return [(k, random_tree(T, rs, k)) for k in ("random", "chain", "star")]


# ============================================================================= 2. accept scan
def ref_accept(tree, spec, sampled, eos, n, tokens_all):
    """dynamic:283-309 in its mask-sum form.  Returns the expected state of every buffer the kernel is handed."""
    ok = sampled[tree.parents] == spec
    ok[0] = True
    got = (ok[None, :] & tree.mask).sum(-1)
    path = np.nonzero(got == tree.depth + 1)[0]
    a = len(path)
    bonus = int(sampled[path[-1]])
    toks = [int(t) for t in spec[path]] + [bonus]
    e = next((i for i, t in enumerate(toks) if t in eos), -1)
    keep = e if e >= 0 else a
    tokens = tokens_all.copy()
    tokens[n:n + a + 1] = toks
    out = np.full(8, SENT, dtype=np.int32)
    out[:5] = [keep, bonus, int(e >= 0), n + keep, a]
    pth = np.full(tree.T + 3, SENT, dtype=np.int32)
    pth[:keep] = path[:keep]
    return dict(out=out, path=pth, tokens=tokens, n=n + keep)


def walk_accept(tree, spec, sampled):
    """brute force: a node is accepted iff every node on root..node matches its parent's sample"""
    acc = []
    for v in range(tree.T):
        c, ok = v, True
        while c != 0:
            p = int(tree.parents[c])
            ok &= sampled[p] == spec[c]
            c = p
        if ok:
            acc.append(v)
    return acc


def model_accept(tree, spec, sampled, eos, n, tokens_all, drop_wave_prefix=False):
    """the kernel's formulation (parent walk, per-wave ordered compaction), on the CPU, for the mutation check: with
    drop_wave_prefix every wave writes its accepted nodes from slot 0"""
    ok = np.zeros(1024, dtype=bool)
    ok[walk_accept(tree, spec, sampled)] = True
    spath = np.zeros(1024, dtype=np.int64)
    base = 0
    for wv in range(16):
        ids = np.nonzero(ok[wv * 64:(wv + 1) * 64])[0] + wv * 64
        at = 0 if drop_wave_prefix else base
        spath[at:at + len(ids)] = ids
        base += len(ids)
    a = base
    bonus = int(sampled[spath[a - 1]])
    toks = [int(spec[spath[i]]) for i in range(a)] + [bonus]
    e = next((i for i, t in enumerate(toks) if t in eos), -1)
    keep = e if e >= 0 else a
    tokens = tokens_all.copy()
    tokens[n:n + a + 1] = toks
    out = np.full(8, SENT, dtype=np.int32)
    out[:5] = [keep, bonus, int(e >= 0), n + keep, a]
    pth = np.full(tree.T + 3, SENT, dtype=np.int32)
    pth[:keep] = spath[:keep]
    return dict(out=out, path=pth, tokens=tokens, n=n + keep)


def check_accept(got, exp, what=""):
    assert got["out"].tolist() == exp["out"].tolist(), (what, "out5 [keep, bonus, eos_hit, n + keep, a]")
    assert np.array_equal(got["path"], exp["path"]), (what, "path (entries from keep on stay sentinel)")
    assert np.array_equal(got["tokens"], exp["tokens"]), (what, "tokens_all, whole buffer")
    assert got["n"] == exp["n"], (what, "*n_ptr")


def steer(tree, spec, v, rs):
    """sampled such that exactly the chain root..v is accepted"""
    sampled = (BASE + rs.randint(0, ALPHA, size=tree.T)).astype(np.int32)
    chain = tree.chain(v)
    for c in chain[1:]:
        sampled[tree.parents[c]] = spec[c]
    sampled[v] = NOMATCH
    return sampled, chain


EOS_KINDS = ["absent", "pos0", "middle", "last", "bonus", "twice"]


def eos_list(kind, n_eos, toks, rs):
    a = len(toks) - 1
    real = {"absent": [], "pos0": [toks[0]], "middle": [toks[a // 2]], "last": [toks[a - 1]], "bonus": [toks[a]],
            "twice": [toks[a // 2], toks[a - 1]]}[kind]
    n_eos = max(n_eos, len(real), 1)
    out = real + [-11 - i for i in range(n_eos - len(real))]
    return [int(out[i]) for i in rs.permutation(len(out))]


def accept_cases(tree, spec, rs):
    """dict(sampled, eos, n, pad, chain | None, label) -- steered and random, EOS kind / n_eos / n cycled over them"""
    T = tree.T
    targets = {0, T - 1, int(np.argmax(tree.depth))}
    for wv in range((T + 63) // 64):                                # one target in every wave of the block
        targets.add(int(rs.randint(wv * 64, min(T, (wv + 1) * 64))))
    depths = np.unique(tree.depth)
    for d in depths[np.linspace(0, len(depths) - 1, min(len(depths), 25)).astype(int)]:   # every depth (up to 25 of them)
        targets.add(int(rs.choice(np.nonzero(tree.depth == d)[0])))
    cyc = 0
    for v in sorted(targets):
        sampled, chain = steer(tree, spec, v, rs)
        toks = [int(t) for t in spec[chain]] + [NOMATCH]
        yield dict(sampled=sampled, eos=eos_list(EOS_KINDS[cyc % 6], (1, 2, 4)[cyc % 3], toks, rs), n=(0, 1, 37, 53)[cyc % 4],
                   pad=0 if cyc % 4 == 3 else 5, chain=chain, label=f"steered v={v} eos={EOS_KINDS[cyc % 6]}")
        cyc += 5                                                    # 5 is coprime to 6, 3 and 4: every combination comes up
    for r in range(8):
        sampled = (BASE + rs.randint(0, ALPHA, size=T)).astype(np.int32)
        eos = [int(BASE + rs.randint(ALPHA))] if r % 2 else [-11]
        eos += [-12 - i for i in range((1, 2, 4)[r % 3] - 1)]
        yield dict(sampled=sampled, eos=eos, n=(0, 1, 37, 53)[r % 4], pad=0 if r % 4 == 3 else 5, chain=None, label=f"random {r}")


def token_buffer(case, spec):
    """history and tail are distinct sentinels; pad == 0 puts n + T (the bonus slot of a fully accepted tree) last"""
    buf = (-1000 - np.arange(case["n"] + len(spec) + 1 + case["pad"])).astype(np.int32)
    buf[case["n"]:case["n"] + len(spec)] = spec
    return buf


def gpu_accept(dev, tree, parents_d, case, spec):
    from umbrella_amd import _lib
    td = _i32(token_buffer(case, spec), dev)
    nd = _i32([case["n"]], dev)
    out = torch.full((8,), SENT, dtype=torch.int32, device=dev)
    pth = torch.full((tree.T + 3,), SENT, dtype=torch.int32, device=dev)
    _lib.call("umb_accept_scan", _i32(case["sampled"], dev), parents_d, td, nd, tree.T, _i32(case["eos"], dev), len(case["eos"]),
              out, pth)
    return dict(out=out.cpu().numpy(), path=pth.cpu().numpy(), tokens=td.cpu().numpy(), n=int(nd.cpu()))


@gpu
@pytest.mark.parametrize("T", ACCEPT_T)
def test_accept_scan_exact(dev, T):
    """out5, the whole path buffer, the whole token buffer and *n_ptr, for steered chains ending in every wave / at every
    depth, random samples with frequent partial matches, every EOS placement, n_eos 1 / 2 / 4 and n up to the buffer's end."""
    from conftest import report_fact
    count = 0
    for kind, tree in accept_trees(T):
        rs = np.random.RandomState(7 * T + len(kind))
        spec = draft_tokens(tree.parents, rs)
        parents_d = _i32(tree.parents, dev)
        for case in accept_cases(tree, spec, rs):
            exp = ref_accept(tree, spec, case["sampled"], case["eos"], case["n"], token_buffer(case, spec))
            if case["chain"] is not None:
                assert exp["out"][4] == len(case["chain"])
            check_accept(gpu_accept(dev, tree, parents_d, case, spec), exp, (T, kind, case["label"]))
            count += 1
    report_fact(f"tree_control/accept cases T={T}", count)


@gpu
def test_accept_scan_chain_of_1024_accepted_whole(dev):
    """CONTRACT (include/umbrella_hip.h): T = 1024 is allowed and a chain accepted whole has a = 1024 -- no thread of the
    1024-thread block has tid == a, so thread 0 carries the bonus token: it lands at tokens_all[n + 1024], takes part in the
    EOS search, and out5 / path / *n_ptr are those of any other tree."""
    tree = random_tree(1024, None, "chain")
    rs = np.random.RandomState(5)
    spec = draft_tokens(tree.parents, rs)
    parents_d = _i32(tree.parents, dev)
    sampled, chain = steer(tree, spec, 1023, rs)
    assert len(chain) == 1024
    for eos in ([-11], [NOMATCH], [-11, int(spec[1023])], [int(spec[500]), NOMATCH, -3, -4]):
        for n, pad in ((0, 0), (37, 5)):
            case = dict(sampled=sampled, eos=eos, n=n, pad=pad)
            exp = ref_accept(tree, spec, sampled, eos, n, token_buffer(case, spec))
            assert exp["out"][4] == 1024 and exp["tokens"][n + 1024] == NOMATCH
            check_accept(gpu_accept(dev, tree, parents_d, case, spec), exp, (eos, n))


@gpu
def test_accept_scan_rejects_bad_tree_sizes(dev):
    from umbrella_amd import _lib
    z = torch.full((1100,), SENT, dtype=torch.int32, device=dev)
    bufs = [z.clone() for _ in range(6)]
    nd = _i32([3], dev)
    for T in (0, 1025, -1):
        with pytest.raises(RuntimeError):
            _lib.call("umb_accept_scan", bufs[0], bufs[1], bufs[2], nd, T, bufs[3], 1, bufs[4], bufs[5])
    torch.cuda.synchronize()
    assert all(torch.equal(b, z) for b in bufs) and int(nd.cpu()) == 3         # nothing was launched


# ============================================================================= 3. beam expand
BEAM_SHAPES = [(1, 1, 1), (1, 16, 16), (1, 32, 32), (3, 5, 15), (16, 24, 16), (21, 24, 21), (32, 32, 32), (64, 16, 64), (64, 16, 1)]
SINGLE_LEVEL_CEILING = 1e-5             # the tolerance of test_beam_expand_matches_reference_trace


def ref_beam(top_val, parent_score, dt=np.float64):
    """dynamic:236-241: log(softmax(top_val) + 1e-4) + tree_score[parent]; order = (score descending, flat index ascending)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        tv = top_val.astype(dt)
        e = np.exp(tv - tv.max(axis=1, keepdims=True))
        cand = (parent_score.astype(dt)[:, None] + np.log(e / e.sum(axis=1, keepdims=True) + dt(1e-4))).reshape(-1)
    return cand, np.argsort(-cand, kind="stable")


def ref_beam_fp32(top_val, parent_score):
    """the reference's own lines in fp32 torch"""
    tv = torch.from_numpy(top_val.astype(np.float32))
    cand = (torch.from_numpy(parent_score.astype(np.float32))[:, None] + torch.log(tv.softmax(dim=-1) + 1e-4)).reshape(-1)
    return cand.numpy()


def beam_offsets(w, W):
    """lvl_off such that the children [lvl_off + w, lvl_off + w + W) start at, end at and straddle bits 63 / 64, 127 / 128, 767 / 768"""
    offs = {0 if w == 1 else 1}
    for b in (64, 128, 768):
        for lo in (b, b - W, b - W // 2, b - 1):
            if lo - w >= 0:
                offs.add(lo - w)
    return sorted(offs)


def beam_case(w, B, W, lvl_off, extra_words, rs, kind="random"):
    T = lvl_off + w + W
    words = (T + 63) // 64 + extra_words
    tv = np.sort((3.0 * rs.randn(w, B)).astype(np.float32), axis=1)[:, ::-1].copy()
    score = rs.randn(T).astype(np.float32) - 4.0
    t0 = max(1, min((W - 1) // w, B - 2))        # beam positions from t0 on form the tied tail; w * t0 < W puts it inside the selection
    if kind == "tie_equal":                       # equal parents, identical rows, equal pairs inside a row: exact ties everywhere
        tv[:, 1::2] = tv[:, 0::2][:, :B // 2]
        tv[:] = tv[0]
        score[lvl_off:lvl_off + w] = score[lvl_off]
    elif kind == "tie_underflow":                 # p underflows to 0 in the tail: those candidates score log(1e-4) + parent exactly
        tv[:, t0:] -= 1000.0                      # (t0 == 1: the heads have p == 1 exactly and tie as well)
        score[lvl_off:lvl_off + w] = score[lvl_off]
    elif kind == "tie_inf":                       # a vocabulary masked to fewer than B finite logits; parents equal in pairs
        tv[:, t0:] = -np.inf
        score[lvl_off:lvl_off + w] = np.repeat(score[lvl_off:lvl_off + (w + 1) // 2], 2)[:w]
    top_idx = np.stack([rs.permutation(50000)[:B] for _ in range(w)]).astype(np.int32)
    n = int(rs.randint(0, 40))
    return dict(w=w, B=B, W=W, lvl_off=lvl_off, words=words, T=T, n=n, kind=kind, top_val=tv, top_idx=top_idx, score=score,
                parents=(-5 - np.arange(T)).astype(np.int32), tokens=(-1000 - np.arange(n + T + 4)).astype(np.int32),
                mask=rs.randint(0, 2 ** 63, size=(T, words), dtype=np.int64).view(np.uint64) * np.uint64(2) +
                rs.randint(0, 2, size=(T, words)).astype(np.uint64))       # random over ALL 64 bits of ALL words


def beam_cases():
    for si, (w, B, W) in enumerate(BEAM_SHAPES):
        rs = np.random.RandomState(300 + si)
        for oi, off in enumerate(beam_offsets(w, W)):
            yield beam_case(w, B, W, off, (0, 3)[oi % 2], rs)
            if oi == 0:
                yield beam_case(w, B, W, off, 3, rs)
        for kind in ("tie_equal", "tie_underflow", "tie_inf"):
            if w * B > 1:
                yield beam_case(w, B, W, beam_offsets(w, W)[-1], 1, rs, kind)


def measured_drift(cases):
    worst = 0.0
    for c in cases:
        p = c["score"][c["lvl_off"]:c["lvl_off"] + c["w"]]
        worst = max(worst, float(np.abs(ref_beam(c["top_val"], p)[0] - ref_beam_fp32(c["top_val"], p)).max()))
    return worst


def beam_groups(cand, order, tol):
    """group id per sorted position: neighbours whose float64 gap is <= tol share a group"""
    s = cand[order]
    return np.concatenate([[0], np.cumsum(np.diff(-s) > tol)])


def model_beam(c, word0_only=False):
    """the kernel's documented result computed from ref_beam in fp32 rounding (mutation check: parent row copied for word 0 only)"""
    lo = c["lvl_off"] + c["w"]
    cand, order = ref_beam(c["top_val"], c["score"][c["lvl_off"]:lo])
    score, parents, tokens, mask = c["score"].copy(), c["parents"].copy(), c["tokens"].copy(), c["mask"].copy()
    for r in range(c["W"]):
        f = int(order[r])
        par = c["lvl_off"] + f // c["B"]
        score[lo + r], parents[lo + r], tokens[c["n"] + lo + r] = cand[f], par, c["top_idx"].reshape(-1)[f]
        row = mask[par].copy()
        if word0_only:
            row[1:] = 0
        row[(lo + r) >> 6] |= np.uint64(1) << np.uint64((lo + r) & 63)
        mask[lo + r] = row
    return dict(score=score, parents=parents, tokens=tokens, mask=mask)


def check_beam(got, c, tol, what=""):
    """-> (children checked exactly, children checked by membership in their near-tie group)"""
    w, B, W, off, n = c["w"], c["B"], c["W"], c["lvl_off"], c["n"]
    lo = off + w
    cand, order = ref_beam(c["top_val"], c["score"][off:lo])
    grp = beam_groups(cand, order, tol)
    pos_of = np.empty(w * B, dtype=np.int64)
    pos_of[order] = np.arange(w * B)
    # untouched ranges, bit for bit
    keep = np.ones(c["T"], dtype=bool)
    keep[lo:lo + W] = False
    assert np.array_equal(got["score"][keep].view(np.uint32), c["score"][keep].view(np.uint32)), (what, "tree_score outside the children")
    assert np.array_equal(got["parents"][keep], c["parents"][keep]), (what, "parents outside the children")
    assert np.array_equal(got["mask"][keep], c["mask"][keep]), (what, "mask rows outside the children")
    tk = np.ones(len(c["tokens"]), dtype=bool)
    tk[n + lo:n + lo + W] = False
    assert np.array_equal(got["tokens"][tk], c["tokens"][tk]), (what, "tokens_all outside the children")
    # scores: the r-th best of the kernel against the r-th best of the float64 reference
    err = np.abs(got["score"][lo:lo + W].astype(np.float64) - cand[order[:W]])
    assert np.all(err <= tol), (what, "score", float(err.max()), tol)
    exact = member = 0
    flats = set()
    for r in range(W):
        par = int(got["parents"][lo + r])
        assert off <= par < lo, (what, r, "parent outside the level")
        hit = np.nonzero(c["top_idx"][par - off] == got["tokens"][n + lo + r])[0]
        assert len(hit) == 1, (what, r, "child token is not one of its parent's top-B")
        f = (par - off) * B + int(hit[0])
        flats.add(f)
        alone = (r == 0 or grp[r] != grp[r - 1]) and (r == w * B - 1 or grp[r] != grp[r + 1])
        if alone:
            assert f == order[r], (what, r, "wrong candidate at this rank", f, int(order[r]))
            exact += 1
        elif c["kind"] != "random" and cand[order[r]] == cand[f]:   # an EXACT tie made on purpose: flat-index order, no freedom
            assert f == order[r], (what, r, "exact tie not in flat-index order", f, int(order[r]))
            exact += 1
        else:
            assert grp[pos_of[f]] == grp[r], (what, r, "candidate from outside the near-tie group")
            member += 1
        row = c["mask"][par].copy()
        row[(lo + r) >> 6] |= np.uint64(1) << np.uint64((lo + r) & 63)
        assert np.array_equal(got["mask"][lo + r], row), (what, r, "mask row != parent row | own bit, over all words")
    assert len(flats) == W, (what, "a candidate was selected twice")
    return exact, member


def gpu_beam(dev, c, top=None):
    from umbrella_amd import _lib
    score, parents = torch.from_numpy(c["score"]).to(dev), _i32(c["parents"], dev)
    tokens, nd = _i32(c["tokens"], dev), _i32([c["n"]], dev)
    mask = torch.from_numpy(c["mask"].view(np.int64)).to(dev)
    ti, tv = top if top is not None else (_i32(c["top_idx"].reshape(-1), dev), torch.from_numpy(c["top_val"].reshape(-1)).to(dev))
    _lib.call("umb_beam_expand", ti, tv, c["w"], c["B"], c["W"], c["lvl_off"], score, parents, tokens, nd, mask, c["words"])
    return dict(score=score.cpu().numpy(), parents=parents.cpu().numpy(), tokens=tokens.cpu().numpy(),
                mask=mask.cpu().numpy().view(np.uint64))


def single_level_tol(cases):
    m = measured_drift(cases)
    return m, min(4.0 * m, SINGLE_LEVEL_CEILING)


@gpu
def test_beam_expand_single_level(dev):
    """Every shape x every children range on / across the word boundaries x two row strides, plus the exact-tie inputs.
    Tolerance: 4 x the measured float64-vs-fp32 difference of the reference over these inputs (1.3e-6 -> 5.1e-6), never
    above 1e-5.  At most 2 % of a case's children may be checked by membership only."""
    from conftest import report_fact
    cases = list(beam_cases())
    measured, tol = single_level_tol(cases)
    exact = member = 0
    for c in cases:
        what = (c["w"], c["B"], c["W"], c["lvl_off"], c["words"], c["kind"])
        e, m = check_beam(gpu_beam(dev, c), c, tol, what)
        assert m <= 0.02 * c["W"], (what, "membership-only children", m)
        exact, member = exact + e, member + m
    report_fact("tree_control/beam single level", {"cases": len(cases), "children_exact": exact, "children_membership_only": member,
                                                   "measured_fp64_vs_fp32": measured, "score_tolerance": tol})


@gpu
def test_beam_expand_through_split_topk(dev):
    """End to end once: umb_topk_rows_ws (64 rows, V = 128256, B = 16) feeding umb_beam_expand on the device."""
    from umbrella_amd import _lib
    w, B, W, V = 64, 16, 64, 128256
    rs = np.random.RandomState(41)
    logits = torch.from_numpy((3.0 * rs.randn(w, V)).astype(np.float32))
    tv, ti = logits.topk(B, dim=-1)
    c = beam_case(w, B, W, 640, 0, rs)
    c["top_val"], c["top_idx"] = tv.numpy().copy(), ti.numpy().astype(np.int32)
    d_idx = torch.full((w * B,), SENT, dtype=torch.int32, device=dev)
    d_val = torch.zeros(w * B, dtype=torch.float32, device=dev)
    ws = torch.zeros(4096 + w * 16 * B * 8, dtype=torch.uint8, device=dev)
    _lib.call("umb_topk_rows_ws", d_idx, d_val, logits.to(dev), w, V, B, None, None, None, None, ws, ws.numel())
    got = gpu_beam(dev, c, top=(d_idx, d_val))
    assert np.array_equal(d_val.cpu().numpy().reshape(w, B), c["top_val"]) and np.array_equal(d_idx.cpu().numpy().reshape(w, B), c["top_idx"])
    measured, tol = single_level_tol([c])
    e, m = check_beam(got, c, tol, "split top-k -> beam")
    assert m <= 0.02 * W


@gpu
def test_beam_expand_rejects_bad_shapes(dev):
    from umbrella_amd import _lib
    z = torch.full((4096,), SENT, dtype=torch.int32, device=dev)
    bufs = [z.clone() for _ in range(6)]
    fl = torch.zeros(4096, dtype=torch.float32, device=dev)
    for w, B, W in ((33, 32, 8), (4, 4, 17), (65, 2, 8), (64, 17, 8)):
        with pytest.raises(RuntimeError):
            _lib.call("umb_beam_expand", bufs[0], fl, w, B, W, 1, fl, bufs[1], bufs[2], bufs[3], bufs[4], 2)
    torch.cuda.synchronize()
    assert all(torch.equal(b, z) for b in bufs) and float(fl.abs().sum()) == 0.0


# ---- a whole tree, level after level
CHAINS = {"w16b24d16": (16, 24, 16, 12), "w32b32d24": (32, 32, 24, 11)}          # W, B, depth, seed


def chain_inputs(W, B, depth, seed):
    rs = np.random.RandomState(seed)
    lv = []
    for step in range(depth):
        w = 1 if step == 0 else W
        lv.append(dict(w=w, off=0 if step == 0 else 1 + (step - 1) * W,
                       top_val=np.sort((3.0 * rs.randn(w, B)).astype(np.float32), axis=1)[:, ::-1].copy(),
                       top_idx=np.stack([rs.permutation(50000)[:B] for _ in range(w)]).astype(np.int32)))
    return lv


def ref_chain(levels, W, B, fp32=False):
    """the reference run level after level on its own results -> scores, parents, tokens (tree-relative) and the smallest
    float64 gap between neighbours in the order among the selected candidates and the first one left out"""
    T = W * len(levels) + 1
    score = np.zeros(T, dtype=np.float32 if fp32 else np.float64)
    parents, tokens, min_gap = np.zeros(T, dtype=np.int32), np.full(T, SENT, dtype=np.int32), np.inf
    for L in levels:
        w, off = L["w"], L["off"]
        lo = off + w
        if fp32:
            cand = ref_beam_fp32(L["top_val"], score[off:lo])
            order = np.argsort(-cand, kind="stable")
        else:
            cand, order = ref_beam(L["top_val"], score[off:lo])
        s = cand[order[:W + 1]].astype(np.float64)
        min_gap = min(min_gap, float(np.min(-np.diff(s))))
        score[lo:lo + W] = cand[order[:W]]
        parents[lo:lo + W] = off + order[:W] // B
        tokens[lo:lo + W] = L["top_idx"].reshape(-1)[order[:W]]
    return score, parents, tokens, min_gap


def chain_tolerance(name):
    W, B, depth, seed = CHAINS[name]
    levels = chain_inputs(W, B, depth, seed)
    s64, p64, t64, gap = ref_chain(levels, W, B)
    s32, p32, t32, _ = ref_chain(levels, W, B, fp32=True)
    measured = float(np.abs(s64 - s32).max())
    return levels, (s64, p64, t64), (s32, p32, t32), measured, 4.0 * measured, gap


def gpu_chain(dev, levels, W, B, n, tokens_len):
    """all levels launched back to back, each reading what the previous launch wrote; nothing is copied to the host in between"""
    from umbrella_amd import _lib
    T = W * len(levels) + 1
    words = (T + 63) // 64
    st = dict(score=torch.zeros(T, dtype=torch.float32, device=dev), parents=torch.zeros(T, dtype=torch.int32, device=dev),
              tokens=_i32(-1000 - np.arange(tokens_len), dev), n=_i32([n], dev),
              mask=torch.zeros(T, words, dtype=torch.int64, device=dev), words=words)
    st["mask"][0, 0] = 1
    tops = [(_i32(L["top_idx"].reshape(-1), dev), torch.from_numpy(L["top_val"].reshape(-1)).to(dev)) for L in levels]
    for L, (ti, tv) in zip(levels, tops):
        _lib.call("umb_beam_expand", ti, tv, L["w"], B, W, L["off"], st["score"], st["parents"], st["tokens"], st["n"], st["mask"], words)
    return st


def check_chain(st, ref64, tol, W, depth, n, what=""):
    s64, p64, t64 = ref64
    T = W * depth + 1
    assert np.array_equal(st["parents"].cpu().numpy(), p64), (what, "parents")
    tok = st["tokens"].cpu().numpy()
    exp_tok = (-1000 - np.arange(len(tok))).astype(np.int32)
    exp_tok[n + 1:n + T] = t64[1:]
    assert np.array_equal(tok, exp_tok), (what, "tokens_all, whole buffer")
    err = float(np.abs(st["score"].cpu().numpy().astype(np.float64) - s64).max())
    assert err <= tol, (what, "accumulated score", err, tol)
    tree = Tree(p64)
    assert torch.equal(st["mask"].cpu(), tree.bits), (what, "packed mask != ancestor closure of the resulting parents")
    return tree, err


@gpu
@pytest.mark.parametrize("name", list(CHAINS))
def test_beam_expand_whole_tree_chained(dev, name):
    """depth 16 at w16 b24 (T = 257) and depth 24 at w32 b32 (T = 769, 1024 candidates per level, 13 mask words).  The seeds
    are chosen (test_beam_reference_fp32_agrees_and_tolerances_hold, CPU) so that no selected candidate has a neighbour
    within the tolerance: every (token, parent, rank) of the tree is checked exactly.  Tolerance: 4 x the measured
    accumulated float64-vs-fp32 drift of the reference (1.2e-6 -> 4.8e-6 at d16, 2.6e-6 -> 1.05e-5 at d24)."""
    from conftest import report_fact
    W, B, depth, _ = CHAINS[name]
    levels, ref64, _, measured, tol, gap = chain_tolerance(name)
    assert gap > tol
    st = gpu_chain(dev, levels, W, B, 9, 9 + W * depth + 1 + 4)
    _, err = check_chain(st, ref64, tol, W, depth, 9, name)
    report_fact(f"tree_control/beam chained {name}", {"children_exact": W * depth, "children_membership_only": 0,
                                                     "measured_fp64_vs_fp32": measured, "score_tolerance": tol, "gpu_error": err})


# ============================================================================= 4. KV compaction
def kv_codes(L, H, Lmax, D):
    """int16 codes naming (key, feature).  D * Lmax <= 65536: key * D + d, every element of a slab distinct.  Larger slabs:
    key * 40503 + d * 30011 mod 2^16 -- both multipliers are odd, so for a fixed feature the code is a bijection of the key
    (every key row differs from every other in EVERY feature) and within a row every feature differs.  Each (layer, head)
    adds its own offset; since every slab is compared whole, a row moved inside the wrong slab shows as well."""
    key, d = np.arange(Lmax, dtype=np.int64)[:, None], np.arange(D, dtype=np.int64)[None, :]
    base = key * D + d if D * Lmax <= 65536 else key * 40503 + d * 30011
    ho = (np.arange(L * H, dtype=np.int64) * 12347).reshape(L, H, 1, 1)
    k = ((base[None, None] + ho) & 0xffff).astype(np.uint16).view(np.int16)                     # [L, H, Lmax, D]
    v = ((base[None, None] + ho + 0x8000) & 0xffff).astype(np.uint16).view(np.int16)            # V differs from K everywhere
    vt = np.zeros((L, H, D, Lmax + VT_PAD), dtype=np.int16)
    vt[..., :Lmax] = v.transpose(0, 1, 3, 2)
    return torch.from_numpy(k), torch.from_numpy(vt)


PAD_SENT = 0x5a5a


class CodedCache:
    """pristine semantic codes (k0 [L, H, Lmax, D], v0 [L, H, D, Lmax + pad]) and their raw fragment-order storage with a
    sentinel in the V^T padding; `expected` applies the reference gather to them"""

    def __init__(self, L, H, Lmax, D):
        self.L, self.H, self.Lmax, self.D = L, H, Lmax, D
        self.k0, self.v0 = kv_codes(L, H, Lmax, D)
        self.kr0 = k_to_frag(self.k0).reshape(L, H, Lmax * D)
        self.vr0 = vt_to_frag(self.v0).reshape(L, H, D * (Lmax + VT_PAD))
        self.vr0[..., D * Lmax:] = PAD_SENT

    def expected(self, n_old, path, keep, in_place=False):
        """cache.py:41-49 of the reference on the semantic view: new[n_old + i] = old[n_old + path[i]], i < keep.
        in_place (mutation check only): destinations written one by one, the last first, so that a source is read after it
        was overwritten -- one of the orders an unstaged parallel copy can take."""
        ek, ev = self.kr0.clone(), self.vr0.clone()
        if keep > 0:
            src = n_old + torch.as_tensor(path[:keep], dtype=torch.long)
            dst = n_old + torch.arange(keep)
            if in_place:
                ks, vs = self.k0.clone(), self.v0.clone()
                for s, t in zip(reversed(src.tolist()), reversed(dst.tolist())):
                    ks[:, :, t], vs[:, :, :, t] = ks[:, :, s].clone(), vs[:, :, :, s].clone()
                krows, vrows = ks[:, :, dst], vs[:, :, :, dst]
            else:
                krows, vrows = self.k0[:, :, src], self.v0[:, :, :, src]
            ek[:, :, k_offsets(dst, self.D)] = krows
            ev[:, :, vt_offsets(dst, self.D)] = vrows
        return ek, ev


def check_kv(got_k, got_v, exp_k, exp_v, what=""):
    """whole K and V^T storage of every layer and head, padding included, bit for bit; a mismatch is named"""
    for name, g, e in (("K", got_k, exp_k), ("V^T", got_v, exp_v)):
        if not torch.equal(g, e):
            bad = (g != e).nonzero()
            lyr, h, off = bad[0].tolist()
            raise AssertionError((what, name, f"{len(bad)} elements differ; first: layer {lyr} head {h} storage offset {off}: "
                                  f"code {int(g[lyr, h, off]) & 0xffff:#06x}, expected {int(e[lyr, h, off]) & 0xffff:#06x}"))


def kv_paths(T, rs):
    """name -> (path, keep, raw accept length); every path is ascending with path[0] = 0 and at most 25 nodes long"""
    m = min(T, 24)
    out = {"identity": (list(range(m)), m, m), "keep0": (list(range(m)), 0, 3), "keep1": ([0] + list(range(2, m + 1))[:m - 1], 1, 1)}
    if T > m + 2:
        out["skip"] = (list(range(m // 2)) + list(range(m // 2 + 1, m + 1)), m, m)
        out["shift"] = ([0] + list(range(2, m + 1)), m, m)
        out["eos_truncated"] = ([0] + list(range(2, m + 1)), m // 2, m)
    W, depth = {769: (32, 24), 257: (16, 16)}.get(T, (3, (T - 1) // 3))
    if W * depth + 1 == T:
        tree = level_tree(W, depth, rs)
        deep = tree.chain(T - 1 - int(rs.randint(W)))
        assert len(deep) == depth + 1
        out["deepest"] = (deep, len(deep), len(deep))
    return out


KV_CONFIGS = [  # D, dtype, (L, Hkv), Lmax
    (32, torch.bfloat16, (1, 1), 64), (32, torch.float16, (3, 2), 1024), (64, torch.bfloat16, (4, 8), 1024),
    (64, torch.float16, (1, 1), 4096), (128, torch.bfloat16, (3, 2), 4096), (128, torch.float16, (4, 8), 64),
    (256, torch.bfloat16, (1, 1), 1024), (256, torch.float16, (3, 2), 4096), (128, torch.bfloat16, (4, 8), 4096),
    (256, torch.float16, (4, 8), 1024)]


def kv_cases(Lmax, rs):
    """(T, n_old, name, path, keep, raw): every (T, n_old) that fits, path kinds cycled so each kind meets each T"""
    cyc = 0
    for T in (13, 257, 769):
        paths = kv_paths(T, rs)
        names = sorted(paths)
        for n_old in sorted({0, 1, 31, 32, 33, 1000, Lmax - T}):
            if n_old < 0 or n_old + T > Lmax:
                continue
            for _ in range(3):
                name = names[cyc % len(names)]
                cyc += 1
                yield (T, n_old, name) + paths[name]


class GpuCache:
    def __init__(self, dev, cc, dtype):
        from umbrella_amd.attn.cache import TreeKVCache
        self.cc, self.dev = cc, dev
        self.c = TreeKVCache(cc.L, cc.H, cc.D, cc.Lmax, dev, dtype)
        self.pk, self.pv = cc.kr0.to(dev), cc.vr0.to(dev)
        self.reset()

    def reset(self):
        self.c.k.view(torch.int16).view(self.cc.L, self.cc.H, -1).copy_(self.pk)
        self.c.vt.view(torch.int16).view(self.cc.L, self.cc.H, -1).copy_(self.pv)

    def raw(self):
        return (self.c.k.view(torch.int16).view(self.cc.L, self.cc.H, -1).cpu(), self.c.vt.view(torch.int16).view(self.cc.L, self.cc.H, -1).cpu())


def kv_res(dev, n_old, keep, raw):
    return _i32([keep, 0, int(keep < raw), n_old + keep, raw, SENT, SENT, SENT], dev)


def kv_path_buffer(dev, path, max_path, T):
    """the entries after the path are valid tree indices the kernel must never use"""
    return _i32(list(path) + [T - 1] * (max_path + 4 - len(path)), dev)


@gpu
@pytest.mark.parametrize("D,dtype,LH,Lmax", KV_CONFIGS, ids=lambda v: str(v).replace("torch.", ""))
def test_kv_compact_exact(dev, D, dtype, LH, Lmax):
    """Through TreeKVCache.compact; once per configuration TreeKVCache.gather_kv_incremental must give the same storage."""
    from conftest import report_fact
    cc = CodedCache(LH[0], LH[1], Lmax, D)
    g = GpuCache(dev, cc, dtype)
    rs = np.random.RandomState(D + Lmax)
    count, gathered = 0, False
    for T, n_old, name, path, keep, raw in kv_cases(Lmax, rs):
        max_path = max(len(path), 1)
        g.reset()
        g.c.compact(kv_res(dev, n_old, keep, raw), kv_path_buffer(dev, path, max_path, T), max_path)
        ek, ev = cc.expected(n_old, path, keep if keep > 1 else 0)
        check_kv(*g.raw(), ek, ev, (D, dtype, LH, Lmax, T, n_old, name))
        if name in ("shift", "deepest") and not gathered:
            g.reset()
            g.c.gather_kv_incremental(torch.tensor(path[:keep]) + n_old, n_old)
            check_kv(*g.raw(), ek, ev, ("gather_kv_incremental", T, n_old, name))
            assert g.c.kv_offset == n_old + keep
            gathered = True
        count += 1
    assert gathered or Lmax < 257
    report_fact(f"tree_control/kv compact cases D={D} {str(dtype)[6:]} LH={LH} Lmax={Lmax}", count)


@gpu
def test_kv_compact_contract_violations(dev):
    """res[0] > max_path breaks the documented precondition: the call stays inside `path` and the staging buffer (the first
    max_path nodes move, nothing else is touched).  Bad shapes, and a staging buffer max_path * D * 4 bytes beyond 64 KiB,
    come back as UMB_EINVAL from the entry point with nothing launched."""
    from umbrella_amd import _lib
    cc = CodedCache(2, 2, 1024, 256)
    g = GpuCache(dev, cc, torch.bfloat16)
    path = [0, 2, 3, 5, 8, 9, 11, 12, 14, 20]
    g.c.compact(kv_res(dev, 40, 10, 10), kv_path_buffer(dev, path, 10, 30), 6)
    check_kv(*g.raw(), *cc.expected(40, path, 6), "res[0] = 10 > max_path = 6")
    g.reset()
    res, pth = kv_res(dev, 40, 10, 10), kv_path_buffer(dev, path, 10, 30)
    code = _lib.dtype_code(torch.bfloat16)
    for L, H, D, Lmax, max_path in ((2, 2, 256, 1000, 10), (2, 2, 48, 1024, 10), (2, 2, 512, 1024, 10), (2, 2, 16, 1024, 10),
                                    (2, 2, 256, 1024, 65), (2, 2, 128, 1024, 129), (2, 2, 256, 1024, -1)):
        with pytest.raises(RuntimeError):
            _lib.call("umb_kv_compact", g.c.k, g.c.vt, res, pth, L, H, D, Lmax, max_path, code)
    _lib.call("umb_kv_compact", g.c.k, g.c.vt, res, pth, 2, 2, 256, 1024, 64, code)        # exactly 64 KiB is launchable
    check_kv(*g.raw(), *cc.expected(40, path, 10), "max_path = 64 at D = 256")


# ============================================================================= 5. one iteration, chained
@gpu
@pytest.mark.parametrize("name", list(CHAINS))
def test_one_iteration_chained_eager_and_graph(dev, name):
    """Beam-expanded tree (section 3's chained launches) -> umb_accept_scan -> umb_kv_compact on a coded cache, the compaction
    reading the res / path buffers the scan wrote on the device.  Once eagerly, once as a captured graph replayed with three
    different n / sampled (a whole leaf chain accepted; an EOS truncating it midway; a short chain).  Tokens, n, path and
    caches equal the CPU references run end to end."""
    from umbrella_amd import _lib
    W, B, depth, _ = CHAINS[name]
    levels, ref64, _, _, tol, _ = chain_tolerance(name)
    tree = Tree(ref64[1])
    T, D, Lmax = tree.T, 64, 1024
    cc = CodedCache(2, 2, Lmax, D)
    g = GpuCache(dev, cc, torch.bfloat16)
    rs = np.random.RandomState(3)
    spec = ref64[2].copy()
    spec[0] = 4242                                                   # the root token is history, not a beam child
    leaf = T - 1 - int(rs.randint(W))
    runs = []
    for v, n, eos_at in ((leaf, 100, None), (leaf, 31, depth // 2), (int(tree.chain(leaf)[3]), Lmax - T, None)):
        sampled, chain = steer(tree, spec, v, rs)
        eos = [-11, int(spec[chain[eos_at]])] if eos_at is not None else [-11, -12]
        runs.append((sampled, n, eos))
    tokens_len = Lmax + 8
    st = gpu_chain(dev, levels, W, B, 0, tokens_len)
    check_chain(st, ref64, tol, W, depth, 0, name)
    tree_tokens = st["tokens"][1:T].clone()                          # the children the device grew (tree-relative 1 .. T - 1)
    sampled_d = torch.zeros(T, dtype=torch.int32, device=dev)
    eos_d = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.zeros(8, dtype=torch.int32, device=dev)
    pth = torch.zeros(depth + 1, dtype=torch.int32, device=dev)

    def stage(sampled, n, eos):
        g.reset()
        st["tokens"].copy_(_i32(-1000 - np.arange(tokens_len), dev))
        st["tokens"][n] = 4242
        st["tokens"][n + 1:n + T] = tree_tokens
        st["n"].fill_(n)
        sampled_d.copy_(_i32(sampled, dev)); eos_d.copy_(_i32(eos, dev))
        out.fill_(SENT); pth.fill_(SENT)

    def iteration():
        _lib.call("umb_accept_scan", sampled_d, st["parents"], st["tokens"], st["n"], T, eos_d, 2, out, pth)
        g.c.compact(out, pth, depth + 1)

    def verify(sampled, n, eos, what):
        buf = (-1000 - np.arange(tokens_len)).astype(np.int32)
        buf[n:n + T] = spec
        exp = ref_accept(tree, spec, sampled, eos, n, buf)
        got = dict(out=out.cpu().numpy(), path=np.concatenate([pth.cpu().numpy(), np.full(T + 3 - depth - 1, SENT, dtype=np.int32)]),
                   tokens=st["tokens"].cpu().numpy(), n=int(st["n"].cpu()))
        check_accept(got, exp, what)
        keep = int(exp["out"][0])
        check_kv(*g.raw(), *cc.expected(n, exp["path"][:keep].tolist(), keep if keep > 1 else 0), what)
        return keep

    keeps = []
    for i, r in enumerate(runs):
        stage(*r)
        iteration()
        keeps.append(verify(*r, (name, "eager", i)))
    assert keeps == [depth + 1, depth // 2, 4]
    stage(*runs[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        iteration()                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    stage(*runs[0])
    with torch.cuda.graph(graph):
        iteration()
    for i, r in enumerate(runs):
        stage(*r)
        graph.replay()
        assert verify(*r, (name, "graph", i)) == keeps[i]


# ============================================================================= 6. arg-max / top-k
def ref_topk(rows, k, zero_bug=False):
    """(value descending, index ascending), -0.0 == +0.0: a stable descending sort.  zero_bug (mutation check only): the
    total order of the bit patterns, where +0.0 ranks above -0.0."""
    rows = np.asarray(rows, dtype=np.float32)
    if zero_bug:
        u = rows.view(np.uint32).astype(np.int64)
        key = np.where(u & 0x80000000, 0xffffffff - u, u | 0x80000000)
        return np.argsort(-key, axis=1, kind="stable")[:, :k]
    return np.argsort(-rows, axis=1, kind="stable")[:, :k]


def check_topk(rows, k, idx, val=None, am=None, what=""):
    exp = ref_topk(rows, k)
    if idx is not None:
        assert np.array_equal(idx, exp), (what, "top-k indices", np.argwhere(idx != exp)[:4].tolist())
    if val is not None:
        assert np.array_equal(val, np.take_along_axis(np.asarray(rows, dtype=np.float32), exp, axis=1)), (what, "top-k values")
    if am is not None:
        assert np.array_equal(am, exp[:, 0]), (what, "arg-max")


def special_rows(V, rs):
    """rows the other tests never feed; V >= 8"""
    nz, pz = np.float32(-0.0), np.float32(0.0)
    sub = np.float32(1e-42)                                          # subnormal
    neg = lambda: -np.abs(rs.randn(V)).astype(np.float32) - 1.0      # noqa: E731
    rows = []
    r = np.full(V, pz); r[0::2] = nz; rows.append(r)                 # -0, +0, -0, ...
    r = np.full(V, nz); r[0::2] = pz; rows.append(r)                 # +0, -0, +0, ...
    r = neg(); r[V // 3], r[V // 2] = nz, pz; rows.append(r)         # a -0 / +0 pair above the rest: the lower index first
    r = neg(); r[V // 3], r[V // 2] = pz, nz; rows.append(r)
    r = neg(); r[[V - 2, 5, V // 2]] = np.inf; rows.append(r)        # several +inf: index order
    rows.append(np.full(V, -np.inf, dtype=np.float32))               # all -inf
    r = np.full(V, nz); r[V // 2], r[3] = sub, -sub; r[1::5] = pz; rows.append(r)     # subnormals next to the zeros
    r = np.full(V, -np.inf, dtype=np.float32); r[[6, 2]] = [pz, nz]; rows.append(r)
    for back in (1, 2, 3):                                           # the winner among the last 1 .. 3 elements
        r = neg(); r[V - back] = 5.0; rows.append(r)
    return np.stack(rows).astype(np.float32)


def gpu_topk(dev, rows, k, ws_rows=None):
    from umbrella_amd import _lib
    R, V = rows.shape
    d = torch.from_numpy(rows).to(dev)
    idx = torch.full((R, k), SENT, dtype=torch.int32, device=dev)
    val = torch.zeros(R, k, dtype=torch.float32, device=dev)
    if ws_rows is None:
        _lib.call("umb_topk_rows", idx, val, d, R, V, k, None, None, None, None)
    else:
        ws = torch.zeros(4096 + ws_rows * 16 * k * 8, dtype=torch.uint8, device=dev)
        _lib.call("umb_topk_rows_ws", idx, val, d, R, V, k, None, None, None, None, ws, ws.numel())
        assert int(ws[:4096].sum()) == 0, "row counters did not reset"
    return idx.cpu().numpy(), val.cpu().numpy()


@gpu
@pytest.mark.parametrize("V", [8, 12, 100, 512, 5001, 16384, 128256, 128257])
def test_argmax_topk_special_values(dev, V):
    """signed zeros tie (lower index wins, as torch.argmax on the CPU), +inf in index order, all -inf,
    subnormals, and V % 4 != 0 (the scalar path) with the winner in the last elements."""
    from umbrella_amd import _lib
    rows = special_rows(V, np.random.RandomState(V))
    am = torch.full((len(rows),), SENT, dtype=torch.int32, device=dev)
    _lib.call("umb_argmax_rows", am, torch.from_numpy(rows).to(dev), len(rows), V)
    check_topk(rows, 1, None, None, am.cpu().numpy(), (V, "argmax"))
    assert am.cpu().numpy().tolist() == torch.from_numpy(rows).argmax(-1).tolist()
    for k in (1, 4, 8) + ((64,) if V >= 64 else ()):
        idx, val = gpu_topk(dev, rows, k)
        check_topk(rows, k, idx, val, None, (V, k, "umb_topk_rows"))
        if V >= 16384:
            idx, val = gpu_topk(dev, rows, k, ws_rows=len(rows))
            check_topk(rows, k, idx, val, None, (V, k, "umb_topk_rows_ws"))


@gpu
@pytest.mark.parametrize("R", [769, 1024, 1025])
def test_topk_split_full_counter_range(dev, R):
    """umb_topk_rows_ws at the counters' full range in one launch (769 and 1024 rows), the documented fallback at 1025, at the
    smallest split vocabulary (V = 16384) with k = 64: == umb_topk_rows everywhere, == the CPU reference on a sample of rows."""
    V, k = 16384, 64
    rs = np.random.RandomState(R)
    rows = rs.randn(R, V).astype(np.float32)
    rows[5] = 0.0
    rows[R - 1, V - 1] = rows[R - 1, 0] = 9.0
    ia, va = gpu_topk(dev, rows, k)
    ib, vb = gpu_topk(dev, rows, k, ws_rows=R)
    assert np.array_equal(ia, ib) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
    pick = sorted(set(range(0, R, 37)) | {5, R - 1, R - 2})
    check_topk(rows[pick], k, ib[pick], vb[pick], None, (R, "sampled rows"))


@gpu
@pytest.mark.parametrize("split", [False, True])
def test_topk_child_placement(dev, split):
    """child_cnt 0, k and mixed, child_start non-monotone; tokens_all compared whole"""
    from umbrella_amd import _lib
    R, V, k, n = 9, 16384, 4, 10
    rs = np.random.RandomState(8)
    rows = rs.randn(R, V).astype(np.float32)
    exp_idx = ref_topk(rows, k)
    for cc in ([0] * R, [k] * R, [4, 0, 2, 1, 3, 4, 0, 1, 2]):
        cs = [33, 1, 29, 5, 21, 9, 17, 13, 25]                       # non-monotone, 4 apart: no two rows share a slot
        base = (-1000 - np.arange(64)).astype(np.int32)
        td = _i32(base, dev)
        args = (None, None, torch.from_numpy(rows).to(dev), R, V, k, td, _i32([n], dev), _i32(cs, dev), _i32(cc, dev))
        if split:
            ws = torch.zeros(4096 + R * 16 * k * 8, dtype=torch.uint8, device=dev)
            _lib.call("umb_topk_rows_ws", *args, ws, ws.numel())
        else:
            _lib.call("umb_topk_rows", *args)
        for r in range(R):
            base[n + cs[r]:n + cs[r] + cc[r]] = exp_idx[r, :cc[r]]
        assert np.array_equal(td.cpu().numpy(), base), (split, cc)


# ============================================================================= 7. the one-line helpers
def ref_override(tokens, n, tbl, parents, off, cnt):
    """include/umbrella_hip.h: slots in order; a sibling that already carries the forced token takes the displaced one"""
    t = tokens.copy()
    for i in range(cnt):
        forced = int(tbl[off + i])
        if forced < 0:
            continue
        old = int(t[n + off + i])
        if parents is not None and old != forced:
            sib = np.nonzero((parents[off:off + cnt] == parents[off + i]) & (t[n + off:n + off + cnt] == forced))[0]
            t[n + off + sib[sib != i]] = old
        t[n + off + i] = forced
    return t


@gpu
def test_small_helpers(dev):
    from umbrella_amd import _lib
    # umb_mask_eos: only the named entries change
    rs = np.random.RandomState(2)
    for eos in ([7], [7, 900], sorted(rs.permutation(1000)[:64].tolist()), [5, 5, 9, 5]):
        row = rs.randn(1000).astype(np.float32)
        d = torch.from_numpy(row).to(dev)
        _lib.call("umb_mask_eos", d, _i32(eos, dev), len(eos))
        row[eos] = -np.inf
        assert np.array_equal(d.cpu().numpy().view(np.uint32), row.view(np.uint32)), eos
    d0 = d.clone()
    with pytest.raises(RuntimeError):
        _lib.call("umb_mask_eos", d, _i32(list(range(65)), dev), 65)
    assert torch.equal(d, d0)
    # umb_write_token / umb_set_int
    tok = _i32(-1000 - np.arange(50), dev)
    _lib.call("umb_write_token", tok, _i32([49], dev), _i32([123, 456], dev))
    _lib.call("umb_write_token", tok, _i32([0], dev), _i32([77], dev))
    exp = (-1000 - np.arange(50)).astype(np.int32)
    exp[49], exp[0] = 123, 77
    assert np.array_equal(tok.cpu().numpy(), exp)
    buf = torch.full((5,), SENT, dtype=torch.int32, device=dev)
    _lib.call("umb_set_int", buf[2:], -31)
    assert buf.cpu().tolist() == [SENT, SENT, -31, SENT, SENT]


@gpu
def test_apply_override(dev):
    """cnt = 1024 (a full level) and 1025 (UMB_EINVAL), forced == drafted, two forced siblings under one parent, no parents"""
    from umbrella_amd import _lib
    rs = np.random.RandomState(6)
    cnt, off, n = 1024, 3, 11
    parents = np.concatenate([[0, 0, 0], np.sort(rs.randint(0, 3, size=cnt))]).astype(np.int32)
    tokens = (-1000 - np.arange(n + off + cnt + 5)).astype(np.int32)
    tokens[n + off:n + off + cnt] = 100 + rs.permutation(cnt)                       # siblings distinct
    tbl = np.full(off + cnt + 2, -1, dtype=np.int32)
    sib0 = np.nonzero(parents[off:] == 0)[0]
    tbl[off + sib0[0]] = tokens[n + off + sib0[0]]                                  # forced == drafted
    tbl[off + sib0[1]] = tokens[n + off + sib0[2]]                                  # two forced siblings under one parent, each
    tbl[off + sib0[2]] = tokens[n + off + sib0[1]]                                  # forced to what the other one drafted
    tbl[off + cnt - 1] = tokens[n + off + cnt - 7]                                  # last slot takes a sibling's token
    tbl[off + 500] = 99999                                                          # a token nobody drafted
    for par in (parents, None):
        td = _i32(tokens, dev)
        _lib.call("umb_apply_override", td, _i32([n], dev), _i32(tbl, dev), None if par is None else _i32(par, dev), off, cnt)
        exp = ref_override(tokens, n, tbl, par, off, cnt)
        assert np.array_equal(td.cpu().numpy(), exp), "parents" if par is not None else "no parents"
        if par is not None:
            for p in range(3):
                s = exp[n + off:n + off + cnt][parents[off:] == p]
                assert len(set(s.tolist())) == len(s), "siblings no longer distinct"
    t0 = td.clone()
    with pytest.raises(RuntimeError):
        _lib.call("umb_apply_override", td, _i32([n], dev), _i32(np.full(2000, 5), dev), _i32(np.zeros(2000), dev), off, 1025)
    assert torch.equal(td, t0)


# ============================================================================= 8. CPU self-tests
def test_tree_builders():
    rs = np.random.RandomState(0)
    trees = [level_tree(16, 16, rs), level_tree(32, 24, rs), level_tree(21, 24, rs), random_tree(129, rs), random_tree(65, rs, "chain"),
             random_tree(65, rs, "star"), random_tree(1, rs)]
    assert [t.T for t in trees[:3]] == [257, 769, 505]
    for t in trees:
        for v in rs.randint(0, t.T, size=20):                         # mask == ancestor closure of parents
            row = np.zeros(t.T, dtype=bool)
            row[t.chain(v)] = True
            assert np.array_equal(t.mask[v], row) and t.depth[v] == row.sum() - 1
        assert torch.equal(t.bits, pack_mask_bits(torch.from_numpy(t.mask))) and t.bits.shape == (t.T, (t.T + 63) // 64)
        tok = draft_tokens(t.parents, rs)
        for p in range(t.T):                                          # siblings distinct
            s = tok[1:][t.parents[1:] == p]
            assert len(set(s.tolist())) == len(s)
    lt = trees[1]
    kids = np.bincount(lt.parents[1:], minlength=lt.T)
    assert (kids[1:-32] > 1).any() and (kids[1:-32] == 0).any()       # shared parents and childless nodes
    assert set(lt.depth[1 + 32 * 5:1 + 32 * 6]) == {6}
    cousins = draft_tokens(lt.parents, rs)
    assert len(set(cousins.tolist())) <= ALPHA + 32                   # small alphabet: cousins collide


def test_accept_reference_against_brute_force_and_steering():
    total = 0
    for T in (1, 2, 13, 65, 129, 257):
        for kind, tree in accept_trees(T):
            rs = np.random.RandomState(T)
            spec = draft_tokens(tree.parents, rs)
            off_path_matches = 0
            for case in accept_cases(tree, spec, rs):
                buf = token_buffer(case, spec)
                exp = ref_accept(tree, spec, case["sampled"], case["eos"], case["n"], buf)
                acc = walk_accept(tree, spec, case["sampled"])
                assert exp["out"][4] == len(acc)
                if case["chain"] is not None:
                    assert acc == case["chain"], "steering did not produce the chain asked for"
                keep = exp["out"][0]
                assert exp["path"][:keep].tolist() == acc[:keep]
                check_accept(model_accept(tree, spec, case["sampled"], case["eos"], case["n"], buf), exp, (T, kind, case["label"]))
                own = case["sampled"][tree.parents] == spec
                own[0] = True
                off_path_matches += int(own.sum()) - len(acc)
                total += 1
            assert T < 13 or kind == "star" or off_path_matches > 0                      # nodes that match on their own but not through an ancestor
    assert total > 100


def test_accept_eos_placements_are_reached():
    tree = level_tree(16, 16, np.random.RandomState(1))
    rs = np.random.RandomState(2)
    spec = draft_tokens(tree.parents, rs)
    seen = set()
    for case in accept_cases(tree, spec, rs):
        exp = ref_accept(tree, spec, case["sampled"], case["eos"], case["n"], token_buffer(case, spec))
        keep, _, hit, _, a = exp["out"][:5].tolist()
        seen.add(("hit" if hit else "none", "pos0" if keep == 0 else "bonus" if keep == a and hit else "inside" if hit else "-",
                  len(case["eos"])))
        seen.add(("n", case["n"], case["pad"]))
    for want in (("hit", "pos0"), ("hit", "bonus"), ("hit", "inside"), ("none", "-")):
        assert any(s[:2] == want for s in seen), want
    assert {s[2] for s in seen if s[0] in ("hit", "none")} >= {1, 2, 4}
    assert {("n", 0, 5), ("n", 1, 5), ("n", 37, 5), ("n", 53, 0)} <= seen


def test_beam_reference_fp32_agrees_and_tolerances_hold():
    """Where the tolerance and the 2 % cap are established, with the references alone: float64 reference vs the reference's
    own lines in fp32 torch make the same selection outside the declared near-tie groups, on every input the GPU tests use."""
    cases = list(beam_cases())
    measured, tol = single_level_tol(cases)
    assert 0 < measured < 2.5e-6 and tol <= SINGLE_LEVEL_CEILING
    kinds = defaultdict(int)
    for c in cases:
        off, lo, W = c["lvl_off"], c["lvl_off"] + c["w"], c["W"]
        cand, order = ref_beam(c["top_val"], c["score"][off:lo])
        c32 = ref_beam_fp32(c["top_val"], c["score"][off:lo])
        o32 = np.argsort(-c32, kind="stable")
        grp = beam_groups(cand, order, tol)
        n = len(order)
        alone = np.array([(r == 0 or grp[r] != grp[r - 1]) and (r == n - 1 or grp[r] != grp[r + 1]) for r in range(W)])
        assert np.array_equal(order[:W][alone], o32[:W][alone])
        if c["kind"] == "random":
            assert (~alone).sum() <= 0.02 * W, ((c["w"], c["B"], W, off), int((~alone).sum()))
        else:
            s = cand[order]
            tied = np.diff(s) == 0
            assert tied[:W].any(), "the tie inputs do not tie inside the selection"
            assert np.all((-np.diff(s) > tol) | tied), "a near (not exact) tie in a tie case"
            exact_f32 = c32[order]
            assert np.all((np.diff(exact_f32) == 0) == tied), "fp32 breaks or makes a tie the float64 reference does not have"
        kinds[c["kind"]] += 1
        # every word boundary case is there
        assert c["words"] >= (c["T"] + 63) // 64
    assert set(kinds) == {"random", "tie_equal", "tie_underflow", "tie_inf"}
    los = {(c["w"], c["W"], c["lvl_off"] + c["w"]) for c in cases}
    for b in (64, 128, 768):
        assert (32, 32, b) in los and (32, 32, b - 32) in los and (32, 32, b - 16) in los
    assert max(c["words"] for c in cases) >= 13
    for name, (W, B, depth, _) in CHAINS.items():
        levels, r64, r32, m, t, gap = chain_tolerance(name)
        assert gap > t, (name, "seed has a near tie among the selected candidates", gap, t)
        assert np.array_equal(r64[1], r32[1]) and np.array_equal(r64[2], r32[2])
        assert m < 8e-6


def test_kv_codes_name_every_row():
    for L, H, Lmax, D in ((1, 1, 64, 32), (3, 2, 1024, 64), (1, 1, 4096, 256)):
        k, vt = kv_codes(L, H, Lmax, D)
        ku = k.numpy().view(np.uint16)
        if D * Lmax <= 65536:
            assert len(np.unique(ku[0, 0])) == D * Lmax
        for d in (0, D - 1):
            assert len(np.unique(ku[0, 0, :, d])) == Lmax             # a key row differs from every other in every feature
        assert len(np.unique(ku[0, 0, 5])) == D
        assert not np.array_equal(ku[0, 0], ku[-1, -1]) or L * H == 1
        assert (vt[..., Lmax:] == 0).all()


def test_engines_size_max_path_to_the_deepest_chain():
    """umb_kv_compact's precondition res[0] <= max_path: the static engine passes len(roots), the dynamic one depth + 1"""
    files = sorted(glob.glob(os.path.join(ROOT, "umbrella_amd", "trees", "*.json")))
    checked = 0
    for f in files + [os.path.join(ROOT, "tests", "golden", "growmaps.json")]:
        with open(f) as fh:
            doc = json.load(fh)
        for gm in ([doc] if isinstance(doc, dict) and "Successors" in doc else [v for v in doc.values() if isinstance(v, dict) and "Successors" in v]
                   if isinstance(doc, dict) else []):
            parents = np.zeros(gm["size"], dtype=np.int32)
            for v, succ in enumerate(gm["Successors"]):
                parents[succ] = v
            assert Tree(parents).depth.max() + 1 <= len(gm["roots"]), f
            checked += 1
    assert checked >= 7
    rs = np.random.RandomState(0)
    for W, depth in ((16, 16), (16, 24), (21, 24), (32, 24)):         # the reference configurations and BASELINE's widest
        assert level_tree(W, depth, rs).depth.max() + 1 == depth + 1


def test_mutations_are_caught():
    """one deliberate defect each, through the assertions the GPU tests use"""
    # accept: wave prefix dropped
    tree = level_tree(32, 24, np.random.RandomState(1))
    rs = np.random.RandomState(2)
    spec = draft_tokens(tree.parents, rs)
    caught = 0
    for case in accept_cases(tree, spec, rs):
        buf = token_buffer(case, spec)
        exp = ref_accept(tree, spec, case["sampled"], case["eos"], case["n"], buf)
        check_accept(model_accept(tree, spec, case["sampled"], case["eos"], case["n"], buf), exp)
        try:
            check_accept(model_accept(tree, spec, case["sampled"], case["eos"], case["n"], buf, drop_wave_prefix=True), exp)
        except AssertionError:
            caught += 1
    assert caught >= 10
    small = random_tree(63, rs)
    sp = draft_tokens(small.parents, rs)
    for case in accept_cases(small, sp, rs):                           # one wave: the defect is invisible, as in the 33-node tests
        buf = token_buffer(case, sp)
        check_accept(model_accept(small, sp, case["sampled"], case["eos"], case["n"], buf, drop_wave_prefix=True),
                     ref_accept(small, sp, case["sampled"], case["eos"], case["n"], buf))
    # beam: parent row copied for word 0 only
    cases = list(beam_cases())
    _, tol = single_level_tol(cases)
    caught = 0
    for c in cases:
        check_beam(model_beam(c), c, tol)
        if c["words"] > 1:
            with pytest.raises(AssertionError, match="mask row"):
                check_beam(model_beam(c, word0_only=True), c, tol)
            caught += 1
    assert caught > 20
    # compact: destination written before the sources are read
    cc = CodedCache(2, 2, 1024, 64)
    caught = {}
    for T, n_old, name, path, keep, raw in kv_cases(1024, np.random.RandomState(3)):
        good = cc.expected(n_old, path, keep if keep > 1 else 0)
        bad = cc.expected(n_old, path, keep if keep > 1 else 0, in_place=True)
        try:
            check_kv(*bad, *good)
            caught.setdefault(name, False)
        except AssertionError:
            caught[name] = True
    assert caught["shift"] and not caught["identity"] and not caught["keep0"]
    # top-k: +0.0 ranked above -0.0
    rows = special_rows(512, np.random.RandomState(4))
    check_topk(rows, 4, ref_topk(rows, 4), None, ref_topk(rows, 1)[:, 0])
    assert ref_topk(rows, 1)[:, 0].tolist() == torch.from_numpy(rows).argmax(-1).tolist()
    with pytest.raises(AssertionError, match="top-k indices"):
        check_topk(rows, 4, ref_topk(rows, 4, zero_bug=True))
    with pytest.raises(AssertionError, match="arg-max"):
        check_topk(rows, 1, None, None, ref_topk(rows, 1, zero_bug=True)[:, 0])
    ordinary = np.random.RandomState(5).randn(4, 512).astype(np.float32)
    check_topk(ordinary, 8, ref_topk(ordinary, 8, zero_bug=True))       # ordinary logits never show it
