"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports
every symbol include/umbrella_hip.h declares; host-side formats round-trip.  No compute calls."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from umbrella_amd import _lib
    return _lib.load()


def test_header_symbols_exported(lib):
    from umbrella_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "umbrella_hip.h")).read()
    declared = set(re.findall(r"\b(umb_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/umbrella_hip.h but not exported"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert lib.umb_version().startswith(b"umbrella_hip")


def test_struct_layouts_match_header(lib):
    """ctypes mirrors must have the C struct sizes (LP64)."""
    import ctypes as C
    from umbrella_amd import _lib
    assert C.sizeof(_lib.UmbLinear) == 56
    assert C.sizeof(_lib.UmbLayer) == 4 * 56 + 24
    assert C.sizeof(_lib.UmbModel) == 10 * 4 + 8 + 8 + 56 + 6 * 8
    assert C.sizeof(_lib.UmbWorkspace) == 16 * 8 + 24 + 8
    assert C.sizeof(_lib.UmbChain) == 18 * 8 + 14 * 4
    assert C.sizeof(_lib.UmbGemmFused) == 144
    assert C.sizeof(_lib.UmbGemmLL) == 152
    assert C.sizeof(_lib.UmbStep) == 8 + 8 * 8 + 6 * 4
    assert C.sizeof(_lib.UmbOffload) == 8 + 8 + 64 + 8 + 64 + 64 + 8 + 8


def test_gemm_plan_is_token_count_free(lib):
    import ctypes as C
    for (N, K, awq) in ((3072, 2048, 0), (128256, 2048, 0), (10240, 8192, 1), (57344, 8192, 1), (8192, 28672, 1)):
        R, S = C.c_int(), C.c_int()
        lib.umb_gemm_plan(N, K, awq, 0, C.byref(R), C.byref(S))
        assert (N // 16) % R.value == 0 and 1 <= S.value <= 16 and (K // 128) >= S.value
        lib.umb_gemm_plan(N, K, awq, 1, C.byref(R), C.byref(S))
        assert S.value == 1


def test_gemm_plan2_balances_whole_rounds(lib):
    """umb_gemm_plan2: tiles per block / waves per block.  The 70B gate/up (3584 n-tiles) runs 256 eight-wave blocks of
    14 tiles (one per CU) instead of 448 four-wave blocks of 8; shapes that already tile the chip keep the round-2 plan."""
    import ctypes as C

    def plan2(N, K, awq, s1=0):
        v = [C.c_int() for _ in range(4)]
        lib.umb_gemm_plan2(N, K, awq, s1, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)
    R, S, tb, srow = plan2(57344, 8192, 1, 1)
    assert (R, S, tb, srow) == (2, 1, 14 | 0x80, 0) and (57344 // 16) // 14 == 256     # one 8-wave block of 14 tiles per CU
    # 8B gate/up (1792 n-tiles = 256 x 7), int4 or dense: one 8-wave block per CU, one tile per wave (round 4)
    assert plan2(28672, 4096, 1, 1) == (1, 1, 7 | 0x80, 0) and plan2(28672, 4096, 0, 1) == (1, 1, 7 | 0x80, 0)
    assert plan2(8192, 8192, 1) == (2, 8, 0, 0)                          # 70B o: the runtime's row-reduce rule caps S at 4
    assert plan2(8192, 28672, 1) == (2, 8, 0, 0)                         # 70B down: 64 x 8 = 512 blocks already
    assert plan2(10240, 8192, 1)[0] == 2 and plan2(10240, 8192, 1)[2] == 0
    for (N, K, awq) in ((3072, 2048, 0), (16384, 2048, 0), (128256, 2048, 0), (6144, 4096, 0)):     # dense: unchanged
        R0, S0 = C.c_int(), C.c_int()
        lib.umb_gemm_plan(N, K, awq, 0, C.byref(R0), C.byref(S0))
        assert plan2(N, K, awq) == (R0.value, S0.value, 0, 0)


def test_ll_plan_is_shape_only_and_consistent(lib):
    """Low-latency GEMM plan (csrc/lowlat.hip): R n-tiles per wave, WN x WK = 8 waves, K-slices of equal length."""
    import ctypes as C
    shapes = [(3072, 2048, 0), (2048, 2048, 0), (16384, 2048, 0), (2048, 8192, 0), (128256, 2048, 0), (6144, 4096, 0),
              (28672, 4096, 1), (4096, 14336, 1), (10240, 8192, 1), (8192, 8192, 1), (57344, 8192, 1), (8192, 28672, 1),
              (384, 256, 0), (256, 128, 0), (512, 256, 1)]
    for (N, K, awq) in shapes:
        v = [C.c_int() for _ in range(4)]
        lib.umb_ll_plan(N, K, awq, *[C.byref(x) for x in v])
        R, WN, WK, NW = (x.value for x in v)
        assert NW == 8 and WN * WK == NW and R in (1, 2)
        assert (N // 16) % R == 0 and (K // 128) % WK == 0
        if awq and R == 2:
            assert (N // 16) % 2 == 0
    assert [lib.umb_ll_token_tiles(t) for t in (0, 1, 16, 17, 32, 33, 48, 49, 64, 65)] == [0, 1, 1, 2, 2, 4, 4, 4, 4, 0]


def test_missing_library_fails_loudly(monkeypatch):
    from umbrella_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libumbrella_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


def test_mask_bit_packing():
    from umbrella_amd.models.llama import pack_mask_bits
    rs = np.random.RandomState(0)
    for T, Cn in ((13, 13), (31, 31), (70, 130), (5, 64), (3, 65)):
        m = torch.from_numpy(rs.rand(T, Cn) > 0.5)
        bits = pack_mask_bits(m)
        assert bits.shape == (T, (Cn + 63) // 64)
        back = torch.zeros(T, Cn, dtype=torch.bool)
        for t in range(T):
            for c in range(Cn):
                back[t, c] = (int(bits[t, c // 64]) >> (c % 64)) & 1
        assert torch.equal(back, m)


def test_sequoia_generator_and_expected_accept():
    import json
    from umbrella_amd.sequoia_utils import expected_accept_length, generate_sequoia_tree
    with open(os.path.join(ROOT, "tests", "golden", "growmaps.json")) as f:
        gm = json.load(f)
    assert generate_sequoia_tree(3, 4) == gm["3x4"]                 # == the reference's shipped 3x4 tree
    assert generate_sequoia_tree(5, 6, gm["5x6_acc"]) == gm["5x6"]
    with open(os.path.join(ROOT, "umbrella_amd", "trees", "sequoia_tree-3x4.json")) as f:
        assert json.load(f) == gm["3x4"]
    e = expected_accept_length(gm["3x4"], [0.65, 0.2, 0.1, 0.05])
    assert 3.0 < e < 3.6


def test_sequoia_generators_do_not_depend_on_the_cpus_log(monkeypatch):
    """The default vector's candidates tie in real arithmetic and are ordered by the last bit of their float32 sums.
    torch.log's vectorised CPU kernels can be one ulp off on some processors (log(0.65f)): with such a log in place both
    generators must still build the reference's shipped trees."""
    import json
    from oracle import sequoia
    from umbrella_amd.sequoia_utils import generate_sequoia_tree
    with open(os.path.join(ROOT, "tests", "golden", "growmaps.json")) as f:
        gm = json.load(f)
    log = torch.log
    monkeypatch.setattr(torch, "log", lambda x, *a, **k: torch.nextafter(log(x, *a, **k), torch.full_like(x, -math.inf)))
    assert generate_sequoia_tree(3, 4) == gm["3x4"]
    assert generate_sequoia_tree(5, 6, gm["5x6_acc"]) == gm["5x6"]
    assert sequoia.generate(3, 4) == gm["3x4"]
    assert sequoia.generate(5, 6, gm["5x6_acc"]) == gm["5x6"]


def test_config_table_and_rope():
    from umbrella_amd.models.config import KNOWN, rope_tables
    c = KNOWN["hugging-quants/Meta-Llama-3.1-70B-Instruct-AWQ-INT4"]
    assert (c.num_hidden_layers, c.hidden_size, c.intermediate_size, c.num_attention_heads, c.head_dim) == (80, 8192, 28672, 64, 128)
    d = KNOWN["meta-llama/Llama-3.2-1B-Instruct"]
    cos, sin = rope_tables(d, 64, torch.bfloat16)
    assert cos.shape == (64, 64) and cos.dtype == torch.bfloat16 and float(cos[0, 0]) == 1.0 and float(sin[0, 0]) == 0.0


def test_gemv_kernels_keep_token_slots_in_registers(tmp_path):
    """hipcc promotes small per-lane arrays that are filled in loops to LDS (8 KiB per block here): the q/k/v GEMV launch
    went from 6.2 to 19.4 us that way.  The kernels without K slices must not use any LDS; the K-sliced one only its
    partial-sum scratch."""
    import re
    import subprocess
    src = os.path.join(ROOT, "umbrella_amd", "csrc", "gemv.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", src, "-o", str(tmp_path / "gemv.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    name = None
    seen = 0
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and name and "gv_kernel" in name:
            seen += 1
            assert int(m.group(1)) <= 1024, (name, int(m.group(1)))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "gv_kernel" in name:
            assert int(m.group(1)) == 0, (name, int(m.group(1)))
    assert seen >= 8


def test_chain_kernels_neither_spill_nor_use_scratch(tmp_path):
    """The persistent chain's consumers hold up to two weight slots and the operand rows in registers across an edge: one
    more inlined copy of the preload code once cost 441 spilled VGPRs and 400 bytes of scratch per lane (1B forward 0.71 ->
    0.97 ms with every parity test green).  With the product's flags no instantiation may spill or touch scratch."""
    import re
    import subprocess
    src = os.path.join(ROOT, "umbrella_amd", "csrc", "chain.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-mllvm",
                        "-amdgpu-kernarg-preload-count=16", "-c", src, "-o", str(tmp_path / "chain.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen = None, 0
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        if not (name and ("draft_chain_kernel" in name or "draft_head_kernel" in name)):
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            seen += 1
            assert int(m.group(1)) == 0, (name, "scratch", int(m.group(1)))
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m:
            assert int(m.group(1)) == 0, (name, "spilled VGPRs", int(m.group(1)))
    assert seen == 6 + 16                 # chain: 2 dtypes x 3 row counts; streamed lm_head: 2 dtypes x 8
