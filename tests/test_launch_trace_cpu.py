"""Which launches the entry points of csrc/mu_api.hip issue, with which arguments, in which order - without a GPU.

mu_api.hip holds no kernel: compiled for the host alone and linked against tests/launch_trace/stubs.hip (every launcher, predicate,
exchange call and HIP runtime call it uses, each as a function that writes its name and arguments down) it runs anywhere.
tests/launch_trace/driver.cpp calls the entry points on states for the three stores, the sparse store's variants and the five kinds of
W update, in the 1..8 and the 9..16 component builds, and prints the trace; the refusals with their codes and messages are part of it.

tests/golden/launch_trace.txt was recorded from mu_api.hip as it stood BEFORE its launch sequencing was gathered into h_half / w_accum /
w_half (the parent commit's file built against these same stubs): the test holds the file to that sequencing, line for line.  A change
that is meant to alter the launches re-records it (driver output of the narrow, then the wide build); `driver --full` prints the
configurations that the file keeps as a line count and a hash (written out they are 78000 lines)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "launch_trace")
BUILDS = [("narrow", []), ("wide", ["-DESPM_KP=16", "-DESPM_MIN_K=9", "-DESPM_MAX_K=16"])]


def _trace(tmp_path, name, defs):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / f"driver_{name}")
    # (host only: no device code is generated, and nothing links the HIP runtime library - the stubs stand in for it)
    flags = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
             "-I", os.path.join(ROOT, "espm_amd", "csrc"), "-I", HERE] + defs
    srcs = (os.path.join(ROOT, "espm_amd", "csrc", "mu_api.hip"), os.path.join(HERE, "stubs.hip"), os.path.join(HERE, "driver.cpp"))
    objs = [str(tmp_path / (name + "_" + os.path.basename(src) + ".o")) for src in srcs]
    compiles = [subprocess.Popen([hipcc] + flags + ["-x", "hip", "-c", src, "-o", obj]) for src, obj in zip(srcs, objs)]
    assert [c.wait() for c in compiles] == [0, 0, 0], "the launch-trace program does not compile"
    subprocess.check_call([os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++"), "-o", exe] + objs)
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout


def test_launch_trace_matches_the_recorded_one(tmp_path):
    got = "".join(_trace(tmp_path, name, defs) for name, defs in BUILDS).splitlines()
    with open(os.path.join(ROOT, "tests", "golden", "launch_trace.txt")) as f:
        want = f.read().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1} of the launch trace: got\n  {g}\nrecorded\n  {w}"
    assert len(got) == len(want)
