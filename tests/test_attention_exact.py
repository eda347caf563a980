"""Tree attention (umbrella_amd/csrc/attn.hip): which keys did each row attend, exactly?

The parity tests elsewhere compare the kernels with an fp32 oracle on N(0, 1) inputs, where the softmax is nearly flat and
one key wrongly included or dropped moves the output by |v| / n_visible -- below their tolerance at long context.  Here:

1. count probes: q = 0 gives every visible key the score 0, so p = 1 / n_vis(t) and, with V a 0/1 code over the keys,
   out[t, h, d] * n_vis(t) is the NUMBER of visible keys whose code has feature d set.  Two codes over a range of 32 D keys
   (residue: (p - a) % D == d; block: (p - a) // 32 == d) name every key by a (block, residue) pair; counts are <= 32.  The
   reference is the bool mask itself.  Margin: p is rounded to the model dtype before P V and the output once more, both
   within 2^-9 relative in bf16 (2^-11 fp16), accumulation is fp32: |out * n_vis - count| <= count * 2^-8 <= 0.125 against
   a rounding threshold of 0.5.  A failing range is re-run with one-hot windows (v[p, d] = 1 iff p == w D + d; out * n_vis
   > 0.5 is the recovered bit) and the (row, head, key) differences are reported.  Rows that see no key at all have no
   defined reference; only the finiteness of their output is asserted.
2. peaked softmax: a target key per row that outscores every other visible key by > 100, placed on tile / span / chunk /
   prefix edges, with HIDDEN decoys that score higher still; and random q scaled by 8.  Oracle: oracle.ops.masked_attention
   (Gemma-2: tests/gemma2_ref.py attention) on fp32 inputs under the tolerances the parity tests use.
3. the FM-ordered output of umb_tree_attn2 is the row-major output, bit for bit.
4. (CPU, no gpu mark) the probes themselves: driven through the oracle they recover the true mask, and a mask with one
   flipped bit makes them fail and name that key.

The CPU tests carry no gpu mark, so the mark is set per test here, not by a module-level pytestmark.
"""
import math

import numpy as np
import pytest
import torch

from oracle import ops as O
from umbrella_amd.attn.cache import VT_PAD, k_to_frag, vt_to_frag

import gemma2_ref as gr

gpu = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
TOL = {torch.bfloat16: 0.03, torch.float16: 0.004}                 # test_hip_ops.py test_tree_attention*
TOL_GEMMA = {torch.bfloat16: 2.5e-2, torch.float16: 4e-3}          # test_gemma2.py test_gemma2_attention_vs_ref


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from umbrella_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------- geometry and expected visibility
def tree_mask(T, rs):
    """random tree in topological order: row i sees itself and its ancestors (as test_hip_ops._tree_mask)"""
    m = torch.zeros(T, T, dtype=torch.bool)
    for i in range(T):
        m[i, i] = True
        if i:
            m[i] |= m[int(rs.randint(0, i))]
    return m


def arbitrary_mask(T, n, rs):
    """not a tree: rows also see LATER keys; one row sees only the very last key, one only key 0, one no mask key at all
    (prefix keys only: with an empty prefix that row sees nothing)"""
    m = torch.from_numpy(rs.rand(T, n) < (0.3 if n <= 64 else 0.05))
    for t in range(T):
        m[t, min(t, n - 1)] = True
    if n > 64:                                   # every combination of bits 63 / 64 (the two sides of a word boundary)
        for t in range(T):
            m[t, 63], m[t, 64] = bool(t & 1), bool(t & 2)
    if T >= 2:
        m[T // 2] = False
        m[T // 2, n - 1] = True
    if T >= 4:
        m[1] = False
        m[1, 0] = True
        m[2] = False
    return m


class Geo:
    """One launch shape.  bits: bool [T, >= n_mask_keys] handed to the kernel as the mask words (None: causal); columns from
    n_mask_keys on are garbage the kernel must ignore.  words: row stride of the mask in 64-bit words.  gemma: None or
    dict(pos int32 [T], window, cap)."""

    def __init__(self, dtype, Hq, Hkv, D, T, prefix, Lmax, bits=None, nmk=None, words=None, chunk=512, counters=True,
                 gemma=None, splits=None):
        self.dtype, self.Hq, self.Hkv, self.D, self.T, self.prefix, self.Lmax = dtype, Hq, Hkv, D, T, prefix, Lmax
        self.bits, self.chunk, self.counters, self.gemma = bits, chunk, counters, gemma
        self.nmk = nmk if nmk is not None else (bits.shape[1] if bits is not None else T)
        self.words = words if words is not None else ((bits.shape[1] + 63) // 64 if bits is not None else 0)
        self.kv_end = prefix + self.nmk
        self.splits = splits if splits is not None else -(-Lmax // chunk)
        self.scale = 1.0 / math.sqrt(D) if gemma is None else (1.0 / 12.0 if D == 128 else 1.0 / 16.0)
        assert self.kv_end <= Lmax and (bits is None or self.nmk <= 64 * self.words)
        assert self.kv_end <= 8192                                    # p = 1 / n_vis stays a normal fp16 number

    @property
    def R(self):
        """keys the count probes cover: the context and 1024 stale slots after it"""
        return min(self.Lmax, self.kv_end + 1024)

    def visible(self, R=None):
        """bool [T, R], written from the contract in include/umbrella_hip.h, not from the kernel"""
        T, R, nmk = self.T, self.R if R is None else R, self.nmk
        vis = torch.zeros(T, R, dtype=torch.bool)
        vis[:, :self.prefix] = True
        if self.bits is not None:
            vis[:, self.prefix:self.kv_end] = self.bits[:, :nmk]
        else:
            vis[:, self.prefix:self.kv_end] = torch.arange(nmk)[None] <= torch.arange(T)[:, None]
        if self.gemma is not None and self.gemma["window"] > 0:
            c = torch.arange(R)[None]
            vis &= (self.gemma["pos"].long()[:, None] - c) < self.gemma["window"]
        return vis

    @property
    def poison(self):
        """Gemma-2: keys before the 32-key tile holding the first key any row's window reaches are never read"""
        if self.gemma is None or self.gemma["window"] <= 0:
            return 0
        return max(int(self.gemma["pos"].min()) - self.gemma["window"] + 1, 0) // 32 * 32


# ----------------------------------------------------------------------------- the probes (device-agnostic)
def code_v(kind, a, D, L, Hkv, dtype, device):
    """V [L, Hkv, D] of 0 / 1: kv head h carries the code rolled by h features, so a head mix-up is a miscount too"""
    rel = torch.arange(L, device=device) - a
    d = torch.arange(D, device=device)[None]
    if kind == "residue":
        hit = ((rel % D)[:, None] == d) & ((rel >= 0) & (rel < 32 * D))[:, None]
    elif kind == "block":
        hit = ((torch.div(rel, 32, rounding_mode="floor"))[:, None] == d) & ((rel >= 0) & (rel < 32 * D))[:, None]
    else:                                        # one-hot window of D keys
        hit = rel[:, None] == d
    V = hit.to(dtype)
    return torch.stack([torch.roll(V, h, dims=1) for h in range(Hkv)], dim=1)


def per_head(base, Hq, Hkv):
    """[T, D] quantity of kv head 0 -> [T, Hq, D] under the per-head roll of code_v"""
    g = Hq // Hkv
    return torch.stack([torch.roll(base, hq // g, dims=-1) for hq in range(Hq)], dim=1)


def count_probe(run, vis, L, Hq, Hkv, D, dtype, poison=0):
    """run(V [L, Hkv, D]) -> out [T, Hq, D] (any float dtype) with q = 0.  Returns (failing ranges, worst |out n - count|
    over rows that see a key).  Asserts every output finite."""
    T, R = vis.shape
    dv = vis.device
    n = vis.sum(1).float()
    live = (n > 0)[:, None, None]
    bad, worst = [], 0.0
    for a in range(0, R, 32 * D):
        for kind in ("residue", "block"):
            V = code_v(kind, a, D, L, Hkv, dtype, dv)
            want = per_head(vis.float() @ V[:R, 0].float(), Hq, Hkv)          # integer counts, exact in fp32
            assert float(want.max()) <= 32
            if poison:
                V[:poison] = float("nan")
            out = run(V).float()
            assert torch.isfinite(out).all(), f"non-finite output (range {a}, {kind} code; never-read keys < {poison})"
            est = out * n[:, None, None]
            ok = (torch.round(est) == want) | ~live
            worst = max(worst, float(((est - want).abs() * live).max()))
            if not bool(ok.all()):
                bad.append((a, kind))
    return bad, worst


def onehot_recover(run, n, lo, hi, L, Hq, Hkv, D, dtype, poison=0):
    """visibility recovered key by key: bool [T, Hq, hi - lo] (lo a multiple of D)"""
    dv = n.device
    g = Hq // Hkv
    cols = []
    for a in range(lo, hi, D):
        V = code_v("onehot", a, D, L, Hkv, dtype, dv)
        if poison:
            V[:poison] = float("nan")
        got = run(V).float() * n[:, None, None] > 0.5                        # feature d of head h <-> key a + (d - h) % D
        cols.append(torch.stack([torch.roll(got[:, hq], -(hq // g), dims=-1) for hq in range(Hq)], dim=1))
    return torch.cat(cols, dim=-1)[..., :hi - lo]


def mask_diff(rec, vis, lo):
    """[(row, head, key, expected bit)] where the recovered visibility differs; rows that see nothing are left out"""
    exp = vis[:, None, lo:lo + rec.shape[-1]].expand_as(rec)
    d = (rec != exp) & (vis.sum(1) > 0)[:, None, None]
    return [(int(t), int(h), int(c) + lo, bool(vis[t, c + lo])) for t, h, c in d.nonzero().tolist()]


def check_visibility(run, vis, L, Hq, Hkv, D, dtype, poison=0, onehot_all=False, what=""):
    bad, worst = count_probe(run, vis, L, Hq, Hkv, D, dtype, poison)
    n = vis.sum(1).float()
    R = vis.shape[1]
    if bad:
        diffs = []
        for a in sorted({a for a, _ in bad}):
            lo, hi = a, min(a + 32 * D, -(-R // D) * D, L)
            vp = torch.cat([vis, torch.zeros(vis.shape[0], max(hi - R, 0), dtype=torch.bool, device=vis.device)], 1)
            diffs += mask_diff(onehot_recover(run, n, lo, hi, L, Hq, Hkv, D, dtype, poison), vp, lo)
        raise AssertionError(f"{what}: wrong key counts in ranges {bad}; (row, q head, key, expected visible) that differ: "
                             f"{diffs[:24]}{' ...' if len(diffs) > 24 else ''} ({len(diffs)} in all)")
    if onehot_all:
        hi = min(-(-R // D) * D, L)
        vp = torch.cat([vis, torch.zeros(vis.shape[0], max(hi - R, 0), dtype=torch.bool, device=vis.device)], 1)
        diffs = mask_diff(onehot_recover(run, n, 0, hi, L, Hq, Hkv, D, dtype, poison), vp, 0)
        assert not diffs, f"{what}: one-hot windows disagree at (row, q head, key, expected visible) {diffs[:24]}"
    return worst


# ----------------------------------------------------------------------------- the kernels behind the probes
class Launch:
    """device buffers of one Geo; run(q, V) is one call of umb_tree_attn2 / umb_tree_attn_gemma2"""

    def __init__(self, geo, dev):
        from umbrella_amd import _lib
        from umbrella_amd.models.llama import pack_mask_bits
        self.g, self.dev, self.lib = geo, dev, _lib
        g = geo
        self.bits = None
        if g.bits is not None:
            full = torch.zeros(g.T, 64 * g.words, dtype=torch.bool)
            full[:, :g.bits.shape[1]] = g.bits
            self.bits = pack_mask_bits(full).contiguous().to(dev)
            assert self.bits.shape == (g.T, g.words)
        self.po = torch.zeros(g.splits * g.T * g.Hq * g.D, dtype=torch.float32, device=dev)
        self.pml = torch.zeros(g.splits * g.T * g.Hq * 2, dtype=torch.float32, device=dev)
        self.pre = torch.tensor([g.prefix], dtype=torch.int32, device=dev)
        nqt = (g.T * (g.Hq // g.Hkv) + 15) // 16
        self.cnt = torch.zeros(g.Hkv * nqt, dtype=torch.int32, device=dev) if g.counters else None
        self.pos = g.gemma["pos"].to(dev) if g.gemma is not None else None
        self.kc = None

    def set_k(self, k):
        """k [Lmax, Hkv, D] (semantic, on the device)"""
        self.kc = k_to_frag(k.permute(1, 0, 2).contiguous())

    def run(self, q, V, fm_tt=0):
        g, lib = self.g, self.lib
        vt = torch.zeros(g.Hkv, g.D, g.Lmax + VT_PAD, dtype=g.dtype, device=self.dev)
        vt[:, :, :g.Lmax] = V.permute(1, 2, 0)
        vt = vt_to_frag(vt)
        rows = 16 * fm_tt if fm_tt else g.T
        out = torch.full((rows, g.Hq, g.D), float("nan"), dtype=g.dtype, device=self.dev)      # unwritten = not finite
        dc = lib.dtype_code(g.dtype)
        if g.gemma is None:
            lib.call("umb_tree_attn2", out, q, self.kc, vt, self.po, self.pml, self.pre, self.bits, g.words, g.nmk, g.T,
                     g.Hq, g.Hkv, g.D, g.Lmax, g.chunk, g.splits, g.scale, self.cnt, fm_tt, dc)
        else:
            lib.call("umb_tree_attn_gemma2", out, q, self.kc, vt, self.po, self.pml, self.pre, self.bits, g.words, g.nmk,
                     g.T, g.Hq, g.Hkv, g.D, g.Lmax, g.splits, g.scale, float(g.gemma["cap"]), self.pos,
                     int(g.gemma["window"]), self.cnt, dc)
        if self.cnt is not None:
            assert int(self.cnt.abs().sum()) == 0                             # the arrival counters reset themselves
        return out


def stale_k(geo, gen, dev):
    """random keys up to kv_end, large finite values in every stale slot after it, NaN where nothing may be read"""
    k = torch.randn(geo.Lmax, geo.Hkv, geo.D, generator=gen)
    k[geo.kv_end:] = 7.0
    k[:geo.poison] = float("nan")
    return k.to(geo.dtype).to(dev)


def gpu_visibility(geo, dev, seed=0, onehot_all=False):
    L = Launch(geo, dev)
    L.set_k(stale_k(geo, torch.Generator().manual_seed(seed), dev))
    q = torch.zeros(geo.T, geo.Hq, geo.D, dtype=geo.dtype, device=dev)
    vis = geo.visible().to(dev)
    assert int((vis.sum(1) == 0).sum()) <= 2
    what = (f"{geo.dtype} Hq {geo.Hq} Hkv {geo.Hkv} D {geo.D} T {geo.T} prefix {geo.prefix} mask keys {geo.nmk} words "
            f"{geo.words} Lmax {geo.Lmax} chunk {geo.chunk} counters {geo.counters} "
            f"{'causal' if geo.bits is None else 'mask'} gemma {geo.gemma and (geo.gemma['window'], geo.gemma['cap'])}")
    return check_visibility(lambda V: L.run(q, V), vis, geo.Lmax, geo.Hq, geo.Hkv, geo.D, geo.dtype, geo.poison,
                            onehot_all, what)


def three_masks(T, nmk, seed):
    """random tree, causal, arbitrary -- [T, nmk] each (None: mask_bits = NULL)"""
    rs = np.random.RandomState(seed)
    n = max(T, nmk)
    tm = tree_mask(n, rs)[n - T:, :nmk] if nmk >= T else tree_mask(T, rs)[:, :nmk]
    return [("tree", tm), ("causal", None), ("arbitrary", arbitrary_mask(T, nmk, rs))]


def llama_cases(dev, dtype, Hq, Hkv, D, T, kv_end, Lmax, seed, **kw):
    prefix = kv_end - T
    worst = 0.0
    for _, bits in three_masks(T, T, seed):
        worst = max(worst, gpu_visibility(Geo(dtype, Hq, Hkv, D, T, prefix, Lmax, bits=bits, **kw), dev, seed))
    return worst


# ----------------------------------------------------------------------------- 1. visibility counts on the GPU
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (8, 1), (4, 4)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kv_end", [1023, 1024, 1025, 1536, 1537, 2049, 4205])
def test_counts_narrow_spans(dev, dtype, Hq, Hkv, D, kv_end):
    """narrow launch with counters: one span up to single_max = 1024 keys, then 512-key spans merged by the last arriver.
    (4, 4): 13 query rows, (32, 8): 52 -- neither fills its last 16-row tile."""
    llama_cases(dev, dtype, Hq, Hkv, D, 13, kv_end, 8192, kv_end + D)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kv_end", [31, 32, 33, 2047, 2048])
def test_counts_one_span_no_counters(dev, dtype, D, kv_end):
    llama_cases(dev, dtype, 8, 2, D, 13, kv_end, 2048, kv_end, counters=False)
    llama_cases(dev, dtype, 12, 4, D, 5, kv_end, 2048, kv_end + 1, counters=False)          # 15 rows per kv head


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("chunk", [256, 512])
@pytest.mark.parametrize("edge", [2, 5])
def test_counts_split_combine(dev, dtype, D, chunk, edge):
    """no counters, Lmax > 2048: key splits of `chunk` keys + attn_combine_kernel; the context ends on a chunk edge and
    one key past it (the last split then holds a single key)"""
    for kv_end in (edge * chunk, edge * chunk + 1):
        llama_cases(dev, dtype, 8, 2, D, 13, kv_end, 8192, kv_end + chunk, chunk=chunk, counters=False)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_counts_split_many_query_tiles(dev, dtype):
    """258 query tiles per kv head: the split kernel walks two query tiles per wave"""
    llama_cases(dev, dtype, 32, 8, 64, 1030, 2049, 8192, 5, chunk=512, counters=False)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,kv_end", [(257, 385), (257, 2557), (769, 897), (769, 3069)])
def test_counts_wide(dev, dtype, T, kv_end):
    """8 kv heads x 129 / 385 query tiles: two waves / one wave per block, 2048-key spans"""
    llama_cases(dev, dtype, 64, 8, 128, T, kv_end, 4096, T + kv_end, chunk=2048)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_counts_head_dim_32(dev, dtype):
    llama_cases(dev, dtype, 4, 4, 32, 13, 1537, 8192, 1)                                    # narrow, four spans
    llama_cases(dev, dtype, 4, 2, 32, 13, 1025, 8192, 2, chunk=256, counters=False)         # split + combine


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nmk", [48, 64, 65, 128, 129])
@pytest.mark.parametrize("T", [1, 3])
def test_counts_draft_level(dev, dtype, nmk, T):
    """the draft-expand call: the last T rows of the tree so far against all its nmk keys, a row stride one word wider
    than needed, and bits past nmk (later levels of a bigger tree) that must be ignored.  nmk <= 64: no end-of-tile scan."""
    rs = np.random.RandomState(nmk * 10 + T)
    N = nmk + 40
    words = (N + 63) // 64 + 1
    for kind in ("tree", "arbitrary"):
        big = tree_mask(N, rs) if kind == "tree" else arbitrary_mask(N, N, rs)
        rows = big[nmk - T:nmk].clone()
        rows[:, nmk:] = torch.from_numpy(rs.rand(T, N - nmk) < 0.5)           # garbage past n_mask_keys
        for prefix, Lmax, counters in ((0, 2048, False), (1000, 8192, True), (1024 - nmk, 8192, True), (1500, 8192, True),
                                       (1500, 8192, False)):
            geo = Geo(dtype, 8, 2, 64, T, prefix, Lmax, bits=rows, nmk=nmk, words=words, counters=counters)
            gpu_visibility(geo, dev, nmk + prefix, onehot_all=(kind == "tree" and prefix == 0 and nmk == 65))
    geo = Geo(dtype, 8, 2, 64, T, 300, 2048, bits=None, nmk=nmk, counters=False)          # causal rows 0 .. T-1 of nmk keys
    gpu_visibility(geo, dev, nmk)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", ["span", "spans", "split"])
@pytest.mark.parametrize("prefix", [0, 64, 65, 121, 124, 127, 1024, 1025, 1081, 1084, 1087])
def test_counts_word_straddle(dev, dtype, path, prefix):
    """prefix % 64 in {0, 1, 57, 60, 63}: the 8 mask bits of a lane come out of two 64-bit words; tree keys 63 and 64 are
    visible in every combination (arbitrary mask), to rows >= 64 (causal) and to their descendants (tree)"""
    T = 70
    Lmax, counters = {"span": (2048, False), "spans": (8192, True), "split": (8192, False)}[path]
    for D, (Hq, Hkv) in ((64, (8, 2)), (128, (4, 4))):
        for kind, bits in three_masks(T, T, prefix + D):
            if kind == "tree":
                bits = bits.clone()
                bits[66:, 63] = bits[66:, 64] = True                              # nodes 66 .. below node 64 below node 63
                bits[64, 63] = bits[65, 63] = bits[65, 64] = True
                bits[66:] |= bits[65]
            geo = Geo(dtype, Hq, Hkv, D, T, prefix, Lmax, bits=bits, counters=counters)
            gpu_visibility(geo, dev, prefix, onehot_all=(D == 64 and kind == "arbitrary" and prefix == 127 and path == "span"))


# ----------------------------------------------------------------------------- Gemma-2
def gemma_tree(T, start, rs):
    """random tree with its depths: rows of different depth share a query tile; pos = start + depth"""
    par = [-1] + [int(rs.randint(0, i)) for i in range(1, T)]
    anc = torch.zeros(T, T, dtype=torch.bool)
    depth = [0] * T
    for i in range(T):
        anc[i, i] = True
        if par[i] >= 0:
            depth[i] = depth[par[i]] + 1
            anc[i] |= anc[par[i]]
    return anc, torch.tensor([start + d for d in depth], dtype=torch.int32)


def gemma_geo(dtype, D, T, start, window, cap, tree, Hq, Hkv, Lmax, seed):
    if tree:
        bits, pos = gemma_tree(T, start, np.random.RandomState(seed))
    else:
        bits, pos = None, torch.arange(start, start + T, dtype=torch.int32)
    return Geo(dtype, Hq, Hkv, D, T, start, Lmax, bits=bits, splits=16, gemma=dict(pos=pos, window=window, cap=cap))


# first key of the shallowest row's window: on a 32-key tile edge (1056) and on a 512-key span edge (1024), one key before
# (the first live tile / span then holds a single visible key of that row) and one after
GEMMA_FIRST = [1023, 1024, 1025, 1055, 1056, 1057]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("window", [16, 64, 700, 0])
def test_counts_gemma2_window_edges(dev, dtype, D, window):
    """expected visibility = mask & (pos[t] - c < window), Geo.visible; keys before the first readable tile are NaN in K
    and V.  Narrow launches (8 waves at D = 128, 4 at D = 256), 512-key spans: span0 > 0 whenever a window is on."""
    Hq, Hkv = (8, 4) if D == 256 else (16, 8)
    for i, first in enumerate(GEMMA_FIRST if window else [1024, 1500]):
        start = first + window - 1 if window else first
        cap = 20.0 if i % 2 else 0.0                                           # tanh(0) = 0: the probe does not change
        for tree in (True, False):
            geo = gemma_geo(dtype, D, 13, start, window, cap, tree, Hq, Hkv, 4096, first + D)
            gpu_visibility(geo, dev, first)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("T,start,window,cap", [(256, 0, 64, 20.0), (256, 1500, 700, 0.0), (900, 0, 64, 0.0),
                                                (900, 1200, 700, 20.0), (900, 300, 0, 20.0)])
def test_counts_gemma2_wide(dev, dtype, D, T, start, window, cap):
    """16 kv heads x 32 / 113 query tiles: two waves / one wave per block, 2048-key spans; causal prompt chunks whose rows'
    windows open on every offset inside a tile"""
    gpu_visibility(gemma_geo(dtype, D, T, start, window, cap, False, 32, 16, 4096, T), dev, T + start)


# ----------------------------------------------------------------------------- 2. peaked softmax with decoys
def peaked_inputs(geo, vis, seed):
    """q [T, Hq, D], k, v [R, Hkv, D] (fp32 values representable in geo.dtype), per-row target keys (-1: none).
    k[tau(t)] = u_t (random signs), q[t] = s u_t with s from the inputs alone so that the target outscores every other
    VISIBLE key by > 100; hidden decoys 1.5 u_t score higher than the target: a masked sibling, a stale slot past kv_end
    and (Gemma-2) the key at pos - window."""
    T, R = vis.shape
    Hq, Hkv, D, dt = geo.Hq, geo.Hkv, geo.D, geo.dtype
    g = Hq // Hkv
    P, E = geo.prefix, geo.kv_end
    edges = [0, P - 1, P, "own", 31, 32, 255, 256, 511, 512, 1023, 1024, 1535, 1536, 2047, 2048, E - 1, "first"]
    for attempt in range(16):
        gen = torch.Generator().manual_seed(seed * 16 + attempt)
        k = (0.1 * torch.randn(R, Hkv, D, generator=gen)).to(dt).float()
        v = torch.randn(R, Hkv, D, generator=gen).to(dt).float()
        tau = [-1] * T
        for t in range(T):
            seen = vis[t].nonzero().flatten()
            if not len(seen):
                continue
            for j in range(len(edges)):
                c = edges[(t + j) % len(edges)]
                c = P + t if c == "own" else int(seen[0]) if c == "first" else c       # "first": first key inside the window
                if 0 <= c < E and vis[t, c]:
                    tau[t] = c
                    break
            else:
                tau[t] = int(seen[-1])
        targets = sorted({c for c in tau if c >= 0})
        sign = torch.where(torch.rand(len(targets), Hkv, D, generator=gen) < 0.5, -1.0, 1.0)
        k[targets] = sign
        used = set(targets)
        for t in range(T):
            if tau[t] < 0:
                continue
            same = torch.tensor([tau[r] == tau[t] for r in range(T)])
            free = ~vis[same].any(0)                                             # hidden from every row aiming at this target
            cands = [c for c in range(tau[t] + 1, min(tau[t] + 40, E)) if c >= P] + [E + (t % 32), E + 32 + (t % 32)]
            if geo.gemma is not None and geo.gemma["window"] > 0:
                cands.insert(0, int(geo.gemma["pos"][t]) - geo.gemma["window"])
            kinds = set()
            for c in cands:
                kind = "stale" if c >= E else "window" if c < tau[t] else "sibling"
                if 0 <= c < R and c >= geo.poison and c not in used and bool(free[c]) and kind not in kinds:
                    k[c] = 1.5 * k[tau[t]]
                    used.add(c)
                    kinds.add(kind)
        rows = [t for t in range(T) if tau[t] >= 0]
        q = torch.randn(T, Hq, D, generator=gen)
        q[rows] = k[[tau[t] for t in rows]].repeat_interleave(g, dim=1)

        def margin(qq):
            s = torch.einsum("thd,chd->thc", qq[rows], k.repeat_interleave(g, dim=1)) * geo.scale
            tgt = torch.stack([s[i, :, tau[t]] for i, t in enumerate(rows)])
            s = s.masked_fill(~vis[rows][:, None, :], float("-inf"))
            for i, t in enumerate(rows):
                s[i, :, tau[t]] = float("-inf")
            return float((tgt - s.amax(-1)).min())
        m1 = margin(q)
        if m1 < 0.5:
            continue                                                            # an unlucky draw of signs: next seed
        q[rows] = (q[rows] * (128.0 / m1)).to(dt).float()
        q = q.to(dt).float()
        assert margin(q) > 100.0 and float(q.abs().max()) < 1024
        return q, k, v, tau
    raise AssertionError("no draw of target vectors separates the targets")


def oracle_attention(geo, q, k, v, vis):
    if geo.gemma is None:
        return O.masked_attention(q, k, v, vis)
    return gr.attention(q, k, v, geo.scale, geo.gemma["cap"], vis)


def gpu_parity(geo, dev, seed, peaked):
    R = min(geo.Lmax, geo.kv_end + 64)                                         # the oracle sees 64 stale slots, all hidden
    vis = geo.visible(R)
    if peaked:
        q, k, v, _ = peaked_inputs(geo, vis, seed)
    else:
        gen = torch.Generator().manual_seed(seed)
        q = (8.0 * torch.randn(geo.T, geo.Hq, geo.D, generator=gen)).to(geo.dtype).float()
        k = torch.randn(R, geo.Hkv, geo.D, generator=gen).to(geo.dtype).float()
        v = torch.randn(R, geo.Hkv, geo.D, generator=gen).to(geo.dtype).float()
    ref = oracle_attention(geo, q, k, v, vis)
    kf = torch.full((geo.Lmax, geo.Hkv, geo.D), 7.0)
    vf = torch.full((geo.Lmax, geo.Hkv, geo.D), -9.0)
    kf[:R], vf[:R] = k, v
    kf[:geo.poison] = float("nan")
    vf[:geo.poison] = float("nan")
    L = Launch(geo, dev)
    L.set_k(kf.to(geo.dtype).to(dev))
    out = L.run(q.to(geo.dtype).to(dev), vf.to(geo.dtype).to(dev)).float().cpu()
    assert torch.isfinite(out).all()
    live = vis.sum(1) > 0                                                      # rows that see nothing: finite is all we ask
    err = float((out - ref)[live].abs().max())
    tol = (TOL if geo.gemma is None else TOL_GEMMA)[geo.dtype]
    assert err < tol, (err, "peaked" if peaked else "q x 8", geo.prefix, geo.T, geo.D, geo.Lmax, geo.counters, geo.chunk)
    return err


PARITY_SHAPES = [
    # (Hq, Hkv, T, kv_end, Lmax, chunk, counters)
    (8, 2, 13, 1000, 8192, 512, True),          # narrow, one span below single_max
    (8, 2, 13, 1537, 8192, 512, True),          # narrow, four 512-key spans, the last with one key
    (8, 2, 13, 4205, 8192, 512, True),
    (8, 2, 13, 2048, 2048, 512, False),         # one 2048-key span, no counters
    (8, 2, 13, 1025, 8192, 256, False),         # key splits + combine
    (8, 2, 13, 2561, 8192, 512, False),
]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("shape", PARITY_SHAPES)
@pytest.mark.parametrize("peaked", [True, False])
def test_peaked_softmax(dev, dtype, D, shape, peaked):
    Hq, Hkv, T, kv_end, Lmax, chunk, counters = shape
    for kind, bits in three_masks(T, T, kv_end + D):
        geo = Geo(dtype, Hq, Hkv, D, T, kv_end - T, Lmax, bits=bits, chunk=chunk, counters=counters)
        gpu_parity(geo, dev, kv_end + D, peaked)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,kv_end", [(257, 2557), (449, 2749)])
@pytest.mark.parametrize("peaked", [True, False])
def test_peaked_softmax_wide(dev, dtype, T, kv_end, peaked):
    """8 kv heads x 129 / 225 query tiles: two waves / one wave per block, two 2048-key spans"""
    for kind, bits in three_masks(T, T, T)[::2]:
        geo = Geo(dtype, 64, 8, 128, T, kv_end - T, 4096, bits=bits, chunk=2048)
        gpu_parity(geo, dev, T, peaked)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("peaked", [True, False])
def test_peaked_softmax_gemma2(dev, dtype, D, peaked):
    """peaked: soft-cap off (a cap of 20 would bound every score difference by 40, and the construction needs > 100);
    q x 8: cap 20, scores far outside tanh's linear range"""
    Hq, Hkv = (8, 4) if D == 256 else (16, 8)
    cap = 0.0 if peaked else 20.0
    for window, first in ((16, 1023), (64, 1024), (64, 1057), (700, 1023), (700, 1025), (0, 1500)):
        start = first + window - 1 if window else first
        for tree in (True, False):
            gpu_parity(gemma_geo(dtype, D, 13, start, window, cap, tree, Hq, Hkv, 4096, first + D), dev, first, peaked)
    gpu_parity(gemma_geo(dtype, D, 256, 1500, 700, cap, False, 32, 16, 4096, 1), dev, 1, peaked)      # two waves
    gpu_parity(gemma_geo(dtype, D, 900, 1200, 700, cap, False, 32, 16, 4096, 2), dev, 2, peaked)      # one wave


# ----------------------------------------------------------------------------- 3. FM-ordered output
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 13, 16, 17, 40, 64])
@pytest.mark.parametrize("prefix", [300, 1500])
def test_fm_output_bit_exact(dev, dtype, D, T, prefix):
    """umb_tree_attn2 writing the o-projection's FM order, converted back by umb_from_fm == the row-major output, bit for
    bit; one span (300 keys) and four spans merged by the last arriver (1500 keys)"""
    from umbrella_amd import _lib
    Hq, Hkv = 8, 2
    gen = torch.Generator().manual_seed(T + prefix + D)
    geo = Geo(dtype, Hq, Hkv, D, T, prefix, 8192, bits=tree_mask(T, np.random.RandomState(T)))
    L = Launch(geo, dev)
    L.set_k(torch.randn(8192, Hkv, D, generator=gen).to(dtype).to(dev))
    q = torch.randn(T, Hq, D, generator=gen).to(dtype).to(dev)
    v = torch.randn(8192, Hkv, D, generator=gen).to(dtype).to(dev)
    rm = L.run(q, v)
    tt = _lib.load().umb_ll_token_tiles(T)
    assert tt * 16 >= T
    fm = L.run(q, v, fm_tt=tt)
    back = torch.empty(T, Hq * D, dtype=dtype, device=dev)
    _lib.call("umb_from_fm", back, fm, T, Hq * D, _lib.dtype_code(dtype))
    assert torch.isfinite(rm.float()).all()
    assert torch.equal(back.view(torch.int16), rm.reshape(T, Hq * D).view(torch.int16))


@gpu
def test_attention_argument_checks(dev):
    """-22: FM output on the split path (no counters, Lmax > 2048) and with too few token tiles; n_mask_keys beyond the
    mask words, through all three entry points"""
    from umbrella_amd import _lib
    dtype, Hq, Hkv, D, T = torch.bfloat16, 8, 2, 64, 17
    bits = tree_mask(T, np.random.RandomState(0))
    for Lmax, counters, fm_tt, ok in ((8192, False, 2, False), (8192, True, 1, False), (2048, False, 1, False),
                                      (8192, True, 2, True), (2048, False, 2, True)):
        L = Launch(Geo(dtype, Hq, Hkv, D, T, 100, Lmax, bits=bits, counters=counters), dev)
        L.set_k(torch.zeros(Lmax, Hkv, D, dtype=dtype, device=dev))
        q, v = torch.zeros(T, Hq, D, dtype=dtype, device=dev), torch.zeros(Lmax, Hkv, D, dtype=dtype, device=dev)
        if ok:
            L.run(q, v, fm_tt=fm_tt)
        else:
            with pytest.raises(_lib.UmbError, match="-22"):
                L.run(q, v, fm_tt=fm_tt)
    # 65 mask keys, one mask word
    geo = Geo(dtype, Hq, Hkv, D, 3, 100, 2048, bits=torch.ones(3, 64, dtype=torch.bool), counters=True)
    L = Launch(geo, dev)
    L.set_k(torch.zeros(2048, Hkv, D, dtype=dtype, device=dev))
    out = torch.zeros(3, Hq, D, dtype=dtype, device=dev)
    q, vt = torch.zeros(3, Hq, D, dtype=dtype, device=dev), torch.zeros(Hkv, D, 2048 + VT_PAD, dtype=dtype, device=dev)
    dc = _lib.dtype_code(dtype)
    for nmk, ok in ((64, True), (65, False), (-1, False)):
        calls = [
            lambda: _lib.call("umb_tree_attn2", out, q, L.kc, vt, L.po, L.pml, L.pre, L.bits, 1, nmk, 3, Hq, Hkv, D, 2048, 512,
                              4, 0.125, L.cnt, 0, dc),
            lambda: _lib.call("umb_tree_attn", out, q, L.kc, vt, L.po, L.pml, L.pre, L.bits, 1, nmk, 3, Hq, Hkv, D, 2048, 512,
                              4, 0.125, L.cnt, dc),
        ]
        for c in calls:
            if ok:
                c()
            else:
                with pytest.raises(_lib.UmbError, match="-22"):
                    c()
    D = 128
    geo = Geo(dtype, Hq, Hkv, D, 3, 100, 2048, bits=torch.ones(3, 64, dtype=torch.bool), splits=16,
              gemma=dict(pos=torch.tensor([100, 101, 102], dtype=torch.int32), window=64, cap=0.0))
    L = Launch(geo, dev)
    L.set_k(torch.zeros(2048, Hkv, D, dtype=dtype, device=dev))
    out, q = torch.zeros(3, Hq, D, dtype=dtype, device=dev), torch.zeros(3, Hq, D, dtype=dtype, device=dev)
    vt = torch.zeros(Hkv, D, 2048 + VT_PAD, dtype=dtype, device=dev)
    for nmk, ok in ((64, True), (65, False)):
        def c():
            _lib.call("umb_tree_attn_gemma2", out, q, L.kc, vt, L.po, L.pml, L.pre, L.bits, 1, nmk, 3, Hq, Hkv, D, 2048, 16,
                      1.0 / 12.0, 0.0, L.pos, 64, L.cnt, dc)
        if ok:
            c()
        else:
            with pytest.raises(_lib.UmbError, match="-22"):
                c()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 4. the probes themselves (CPU)
def _cpu_case(dtype):
    """a 70-node tree behind a 100-key prefix, 86 stale slots after it; the oracle stands in for the kernel"""
    Hq, Hkv, D, T, prefix, L = 4, 2, 64, 70, 100, 256
    rs = np.random.RandomState(7)
    bits = tree_mask(T, rs)
    bits[66:, 63] = bits[66:, 64] = True                    # rows that see tree keys 63 and 64
    geo = Geo(dtype, Hq, Hkv, D, T, prefix, L, bits=bits)
    k = torch.randn(L, Hkv, D, generator=torch.Generator().manual_seed(1)).to(dtype)
    k[geo.kv_end:] = 7.0
    q = torch.zeros(T, Hq, D, dtype=dtype)

    def runner(mask):                                        # the "kernel": the oracle in the model dtype under `mask`
        return lambda V: O.masked_attention(q, k, V.to(dtype), mask)
    return geo, runner


@pytest.mark.parametrize("dtype", DTYPES)
def test_probes_recover_the_mask_through_the_oracle(dtype):
    geo, runner = _cpu_case(dtype)
    vis = geo.visible()
    assert vis.shape == (70, 256) and int(vis.sum(1).min()) > 0
    worst = check_visibility(runner(vis), vis, geo.Lmax, geo.Hq, geo.Hkv, geo.D, dtype, onehot_all=True)
    assert worst < 0.5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row,key", [(5, 17), (69, 100 + 63), (69, 100 + 64), (40, 100 + 63), (40, 100 + 64), (69, 169),
                                     (3, 169), (12, 170), (0, 0), (30, 99), (30, 255)])
def test_probes_name_a_single_flipped_key(dtype, row, key):
    """the oracle computes under a mask with ONE bit flipped (prefix, bits 63 / 64 of the tree, the last key, a stale slot)
    while the expectation keeps the true mask: the count probe fails and the one-hot windows name exactly that key"""
    geo, runner = _cpu_case(dtype)
    vis = geo.visible()
    wrong = vis.clone()
    wrong[row, key] = ~wrong[row, key]
    bad, _ = count_probe(runner(wrong), vis, geo.Lmax, geo.Hq, geo.Hkv, geo.D, dtype)
    assert bad and all(a == 0 for a, _ in bad)
    n = vis.sum(1).float()
    rec = onehot_recover(runner(wrong), n, 0, 256, geo.Lmax, geo.Hq, geo.Hkv, geo.D, dtype)
    assert mask_diff(rec, vis, 0) == [(row, h, key, bool(vis[row, key])) for h in range(geo.Hq)]
    with pytest.raises(AssertionError, match=rf"\({row}, 0, {key}, {bool(vis[row, key])}\)"):
        check_visibility(runner(wrong), vis, geo.Lmax, geo.Hq, geo.Hkv, geo.D, dtype)


def test_peaked_inputs_separate_targets_and_decoys():
    """the construction of section 2, checked against the fp32 oracle alone: every row returns its target's V although
    hidden keys score higher"""
    rs = np.random.RandomState(3)
    pos = torch.arange(1086, 1086 + 13, dtype=torch.int32)
    for geo in (Geo(torch.bfloat16, 8, 2, 32, 13, 1524, 8192, bits=tree_mask(13, rs)),
                Geo(torch.float16, 8, 2, 64, 13, 1012, 8192, bits=arbitrary_mask(13, 13, rs)),
                Geo(torch.bfloat16, 8, 4, 128, 13, 1086, 4096, splits=16, gemma=dict(pos=pos, window=64, cap=0.0))):
        vis = geo.visible()
        q, k, v, tau = peaked_inputs(geo, vis, 11)
        ref = oracle_attention(geo, q, k, v, vis)
        g = geo.Hq // geo.Hkv
        hidden_higher = 0
        for t in range(geo.T):
            if tau[t] < 0:
                continue
            assert torch.equal(ref[t], v[tau[t]].repeat_interleave(g, dim=0))
            s = torch.einsum("hd,chd->hc", q[t], k.repeat_interleave(g, dim=1)) * geo.scale
            hidden_higher += int(((s > s[:, tau[t]][:, None]) & ~vis[t][None]).any())
        assert hidden_higher >= geo.T - 2
