"""How the sparse store's launches lay out a workgroup's LDS (csrc/mu_ell_plan.hpp) - host arithmetic, checked without a GPU.

csrc/mu_ell.hip, mu_h_chain.hip and mu_fused.hip compiled for the host alone and linked against tests/ell_plan/driver.hip (the HIP
runtime's launch, attribute and registration calls, check_hip / set_error and the two lean fused launchers, each as a stub that
writes its arguments down) run anywhere.  A launch leaves one record: the kernel by the name the unit registered for the launched
host pointer, grid, block, dynamic LDS, the LDS granted, every field of the argument block the launcher lays out (h_segs, cnt_ /
meta_ / perm_ / red_lds_off, perm_lds, slab_lds, w_split, cs_lds_off, chain_lds_off, tail_on, the streaming bytes), the return code
and the error text.  The lean launchers are stubs, so for them the instance is pinned as (plain | plain-stream, k, loss, full) - the
arguments they are called with - and not as a kernel name; every other launch is pinned by kernel name.

tests/golden/ell_plan_trace.txt was recorded from the three sources as they stood BEFORE the layouts were gathered into
mu_ell_plan.hpp (the parent commit's files built against this same driver): the test holds the launchers to those layouts, line for
line.  The grid (tests/golden/ell_plan_grid.txt, found by `driver sweep` on the same parent sources, united over the four settings
of the environment knobs): k 1..16; pb 128..1024 (tile_px 64..512); cs_parts, loss and stream_lists on and off, the tail off, riding
and riding with the projected gradient's term; the H-step's three rules; ESPM_FUSED_PLAIN unset / 0 and ESPM_FUSED_SMALL_SEGS unset /
8; n_pad 8, 1000, and the value below and the value above every n_pad (8..16384 in steps of 8) at which anything discrete of a record
changes for that (k, pb) - the kernel, a flag, a segment count, which side of 64 KB or the 160 KB a size lies on, whether the
reduction scratch lies in the table or behind, the return code; at n_pad = 1000 also every fact of the fused launch's common
case turned the other way, one at a time.  The file keeps each (launch, k, pb, knobs) as a line count and a hash; `driver trace
GRID --full` writes them out.  The predicates - fused_ell_lds_bytes with its comparison against ESPM_ELL_LDS_MAX, ell_chain_fits
(through h_chain_built) and espm_mu_ell_h_lds_bytes against what ell.lds_bytes_h computed in Python before it asked the library -
are held to the parent's answers for every n = 1..16384.

    python tests/test_ell_plan_cpu.py --record CSRC INCLUDE    # re-record grid and trace from the sources under CSRC / INCLUDE

tests/golden/ell_plan_h_lds.txt (per k the sha256 of the 16384 answers) was written with h_lds_digest from the Python formula while
ell.lds_bytes_h still was one; the formula is gone, so the file is kept, not re-recorded.
"""
import hashlib
import os
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "ell_plan")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BUILDS = [("narrow", []), ("wide", ["-DESPM_KP=16", "-DESPM_MIN_K=9", "-DESPM_MAX_K=16"])]
KNOBS = [{}, {"ESPM_FUSED_PLAIN": "0"}, {"ESPM_FUSED_SMALL_SEGS": "8"}, {"ESPM_FUSED_PLAIN": "0", "ESPM_FUSED_SMALL_SEGS": "8"}]
UNITS = ("mu_ell.hip", "mu_h_chain.hip", "mu_fused.hip")
N_MAX = 16384


def build_driver(out_dir, name, defs, csrc=os.path.join(ROOT, "espm_amd", "csrc"), include=os.path.join(ROOT, "include")):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = os.path.join(str(out_dir), f"driver_{name}")
    # (host only: no device code is generated and nothing links the HIP runtime library.  -fuse-cuid=none: every unit's registration
    #  then names the same device-image symbol, which the driver defines; each also defines the unit-id symbol, hence muldefs)
    flags = ["--offload-arch=gfx950", "--cuda-host-only", "-fuse-cuid=none", "-O1", "-std=c++17", "-I", include, "-I", csrc] + defs
    srcs = [os.path.join(csrc, u) for u in UNITS] + [os.path.join(HERE, "driver.hip")]
    objs = [os.path.join(str(out_dir), name + "_" + os.path.basename(src) + ".o") for src in srcs]
    compiles = [subprocess.Popen([hipcc] + flags + ["-x", "hip", "-c", src, "-o", obj]) for src, obj in zip(srcs, objs)]
    assert [c.wait() for c in compiles] == [0] * len(srcs), "the layout driver does not compile"
    subprocess.check_call([os.environ.get("CXX", "/opt/rocm/llvm/bin/clang++"), "-Wl,-z,muldefs", "-o", exe] + objs)
    return exe


def run(exe, *args, knobs=None):
    env = {k: v for k, v in os.environ.items() if k not in ("ESPM_FUSED_PLAIN", "ESPM_FUSED_SMALL_SEGS")}
    env.update(knobs or {})
    return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True, env=env).stdout


def trace_text(exes):
    grid = os.path.join(GOLDEN, "ell_plan_grid.txt")
    out = []
    for name, _ in BUILDS:
        for i, knobs in enumerate(KNOBS):
            lines = run(exes[name], "trace", grid, knobs=knobs).splitlines()
            # (the H-step and its chained form read no knob: once per build)
            out += [l for l in lines if i == 0 or l.startswith("fused")]
        out += run(exes[name], "predicates").splitlines()
    return out


def h_lds_digest(lds_bytes_h, k):
    """sha256 of the sparse H-step's LDS bytes for n = 1 .. N_MAX channels (n_pad: n rounded up to 8) at k components."""
    return hashlib.sha256(struct.pack(f"<{N_MAX}q", *(lds_bytes_h((n + 7) // 8 * 8, k) for n in range(1, N_MAX + 1)))).hexdigest()


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("ell_plan")
    return {name: build_driver(out, name, defs) for name, defs in BUILDS}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


def test_the_launches_lay_out_what_the_parent_laid_out(exes):
    got = trace_text(exes)
    with open(os.path.join(GOLDEN, "ell_plan_trace.txt")) as f:
        want = f.read().splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1} of the layout trace: got\n  {g}\nrecorded\n  {w}"
    assert len(got) == len(want)


def test_the_size_query_answers_what_python_computed(lib):
    """espm_mu_ell_h_lds_bytes (include/espm_mu.h) through ell.lds_bytes_h, against the digests of the Python formula it replaced."""
    from espm_amd import ell
    with open(os.path.join(GOLDEN, "ell_plan_h_lds.txt")) as f:
        want = dict(line.split() for line in f)
    assert sorted(want) == [str(k) for k in sorted(range(1, 17), key=str)]
    for k in range(1, 17):
        assert h_lds_digest(ell.lds_bytes_h, k) == want[str(k)], k
    # a build asked for a component count it has no sparse kernels for: (size_t)-1
    none = 2 ** 64 - 1
    assert lib.variant(5).lib.espm_mu_ell_h_lds_bytes(2048, 12) == none and lib.variant(12).lib.espm_mu_ell_h_lds_bytes(2048, 5) == none
    assert lib.variant(20).lib.espm_mu_ell_h_lds_bytes(2048, 20) == none and lib.variant(5).lib.espm_mu_ell_h_lds_bytes(2048, 0) == none


def test_the_gpu_cases_reach_the_shapes_they_claim(exes):
    """tests/ell_plan_cases.py, which tests/test_gpu_ell_plan.py runs: every case reaches its shape, the cases are the smallest
    (k, n_pad) that do, and together they are every shape the fused launch's plan reaches (driver.hip: shape_key)."""
    import ell_plan_cases as ec
    # (a launch that fused_ell_lds_bytes admits and the launcher then refuses would show as a shape "refused": there is none)
    assert run(exes["narrow"], "shapes").splitlines() == [f"k={c['k']} n_pad={c['n_pad']} pb={c['pb']} stream={c['stream']}: {c['shape']}" for c in ec.CASES]
    assert run(exes["wide"], "shapes").splitlines() == ["k=9 n_pad=8 pb=128 stream=0: refused"]   # (the fused launch: 1..8 components)
    for c in ec.CASES:
        out = run(exes["narrow"], "shape", c["k"], c["n_pad"], c["pb"], c["stream"]).splitlines()
        assert out[-1] == "shape: " + c["shape"], (c, out)
        assert " rc=0" in out[1] and "h_step_ell_kernel" in out[1], (c, out)   # the chained H-only launch fits as well


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == "--record":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        built = {name: build_driver(tmp, name, defs, csrc=sys.argv[2], include=sys.argv[3]) for name, defs in BUILDS}
        at = {}
        for name, _ in BUILDS:
            for knobs in KNOBS:
                for line in run(built[name], "sweep", knobs=knobs).splitlines():
                    key, values = line.split(" :")
                    at.setdefault(key, set()).update(int(v) for v in values.split())
        with open(os.path.join(GOLDEN, "ell_plan_grid.txt"), "w") as f:
            for key, values in at.items():
                f.write(key + " : " + " ".join(str(v) for v in sorted(values)) + "\n")
        with open(os.path.join(GOLDEN, "ell_plan_trace.txt"), "w") as f:
            f.write("\n".join(trace_text(built)) + "\n")
