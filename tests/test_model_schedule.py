"""CPU launch trace of umbrella_amd/csrc/model.hip: which launches every forward issues, in which order, with which arguments.

model.hip holds no kernel; it is the host code that picks a schedule and hands operands to the launch functions.  Its
host-only object is linked against the logging stubs of tests/host/model_trace.cpp and every entry point is driven through
that file's case table; stdout must equal tests/golden/model_schedule_trace.txt byte for byte.  The golden file was recorded
with the model.hip of commit 0f7c762 (before the schedules were merged into one driver) and pins that behaviour: a callee,
an argument, a struct field, the order of two launches, a return code.  It cannot see anything inside a kernel."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "umbrella_amd", "csrc", "model.hip")
HARNESS = os.path.join(ROOT, "tests", "host", "model_trace.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "model_schedule_trace.txt")


def _host_cxx(hipcc):
    """A plain C++ compiler for the harness and the link (no HIP runtime library): the clang++ next to hipcc, else c++."""
    root = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for p in (os.path.join(root, "lib", "llvm", "bin", "clang++"), os.path.join(root, "llvm", "bin", "clang++")):
        if os.path.exists(p):
            return p
    return shutil.which("c++") or shutil.which("g++")


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    cxx = _host_cxx(hipcc)
    if not cxx:
        pytest.skip("no host C++ compiler here")
    tmp = tmp_path_factory.mktemp("model_trace")
    obj, hobj, exe = str(tmp / "model.o"), str(tmp / "harness.o"), str(tmp / "model_trace")
    for cmd in ([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O3", "-std=c++17", "-c", SRC, "-o", obj],
                [cxx, "-O1", "-std=c++17", "-c", HARNESS, "-o", hobj],
                [cxx, obj, hobj, "-o", exe]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    groups = subprocess.run([exe, "--groups"], capture_output=True, text=True, check=True).stdout.split()
    assert len(groups) >= 9
    env = {k: v for k, v in os.environ.items() if not k.startswith("UMB_")}
    out = []
    for g in groups:                       # model.hip caches its getenv knobs in statics: one fresh process per setting
        r = subprocess.run([exe, g], capture_output=True, env=env)
        assert r.returncode == 0, (g, r.stderr[-2000:])
        out.append(r.stdout)
    return b"".join(out).decode()


def test_trace_matches_golden(trace):
    golden = open(GOLDEN, newline="").read()
    if trace == golden:
        return
    got, want = trace.split("\n"), golden.split("\n")
    header = "(before the first case)"
    for i in range(max(len(got), len(want))):
        g = got[i] if i < len(got) else "<end of trace>"
        w = want[i] if i < len(want) else "<end of golden file>"
        if g != w:
            pytest.fail(f"launch trace differs from tests/golden/model_schedule_trace.txt at line {i + 1}, in\n  {header}\n"
                        f"golden: {w}\ntrace:  {g}")
        if g.startswith("== "):
            header = g
    pytest.fail("launch trace differs from the golden file")


def test_trace_reaches_every_callee_and_entry_point(trace):
    """Every function model.hip calls outside itself shows in the trace, and every extern "C" entry point is driven."""
    src = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(SRC).read(), flags=re.S)
    entries = set(re.findall(r'extern "C"[^;{(]*?\b(umb_\w+)\s*\(', src))
    called = set(re.findall(r"\b(umb_[a-z0-9_]+|hip[A-Z]\w+)\s*\(", src)) - entries
    assert len(entries) == 8 and len(called) == 36, (sorted(entries), sorted(called))
    first_words = {line.split(" ", 1)[0] for line in trace.split("\n")}
    assert called - first_words <= {"hipGetErrorString"}, sorted(called - first_words)
    driven = set(re.findall(r"^== case \S+ entry=(\w+)$", trace, flags=re.M)) | ({"umb_version"} & first_words)
    assert driven == entries, sorted(entries ^ driven)
