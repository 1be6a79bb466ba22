"""The table of tests/test_gpu_ell_plan.py: one row per distinct shape that the plan of the sparse store's fused launch reaches
(csrc/mu_ell_plan.hpp: plan_fused; DESIGN.md, "LDS of the sparse store's launches"), each at the smallest (k, n_pad) that reaches
it.  tests/test_ell_plan_cpu.py checks the table against the launcher without a GPU - every row reaches its shape, no smaller
(k, n_pad) does, no reachable shape is missing (`driver shapes`) - and the GPU test runs the rows.

A shape, as tests/ell_plan/driver.hip spells it (shape_key): the geometry (full: blocks of 1024 pixels; small: 128 .. 512); the
block's permutations in LDS or not; the record reduction's scratch in the dead part of the table, behind the permutations, or
none; the block's slab in the numerators' region as it is (lds), in the region grown for it (grown), or not in LDS (none); the
copy of colsum(GW') behind (the fused launch has no other place for it: "late" is the H-step's alone, which
test_gpu_estimator.py::test_sparse_store_at_its_lds_limit runs); segments per list group at the floor or above it; the instance.
The launch is the one espm_mu_iterate issues from the second iteration on: the W update's tail rides (cs_parts), with the loss.

A row: k, n_pad (the image has n = n_pad channels), pb (pixels per block; tile_px = pb / 2 is forced), stream (the lists read past
the last-level cache: espm_mu_state.ell_stream, which ESPM_ELL_STREAM_MB=0 sets on any image), the shape.  The image has
2 pb + 37 pixels: two blocks and a ragged third.  The chained H-only launch fits LDS at every row (the CPU test asserts it)."""
import numpy as np


def _row(k, n_pad, pb, stream, shape):
    return dict(id=f"k{k}-n{n_pad}-pb{pb}" + ("-stream" if stream else ""), k=k, n_pad=n_pad, pb=pb, stream=stream, shape=shape)


CASES = [
    _row(1, 8, 128, 0, "small perm_lds=1 red:behind slab:lds cs:behind segs:floor plain"),
    _row(1, 8, 1024, 0, "full perm_lds=0 red:behind slab:lds cs:behind segs:floor plain"),
    _row(1, 8, 1024, 1, "full perm_lds=0 red:behind slab:lds cs:behind segs:floor plain-stream"),
    _row(1, 1032, 128, 0, "small perm_lds=1 red:behind slab:grown cs:behind segs:floor plain"),
    _row(1, 2056, 128, 0, "small perm_lds=1 red:behind slab:grown cs:behind segs:floor generic"),       # more channels than the lean instance stages
    _row(1, 2056, 1024, 0, "full perm_lds=0 red:behind slab:lds cs:behind segs:floor generic"),
    _row(1, 4104, 1024, 0, "full perm_lds=0 red:behind slab:grown cs:behind segs:floor generic"),
    _row(1, 6648, 512, 0, "small perm_lds=1 red:behind slab:none cs:behind segs:floor generic"),        # the region grown for the slab no longer fits
    _row(1, 7752, 512, 0, "small perm_lds=1 red:none slab:none cs:behind segs:floor generic"),          # nor the reduction's own scratch
    _row(1, 8064, 1024, 0, "full perm_lds=0 red:behind slab:none cs:behind segs:floor generic"),
    _row(1, 9048, 1024, 0, "full perm_lds=0 red:none slab:none cs:behind segs:floor generic"),
    _row(5, 8, 1024, 0, "full perm_lds=0 red:behind slab:lds cs:behind segs:above plain"),
    _row(5, 8, 1024, 1, "full perm_lds=0 red:behind slab:lds cs:behind segs:above plain-stream"),
    _row(5, 2056, 1024, 0, "full perm_lds=0 red:behind slab:lds cs:behind segs:above generic"),
    _row(5, 3944, 1024, 0, "full perm_lds=0 red:table slab:lds cs:behind segs:above generic"),          # a fourth segment with the scratch in the table
    _row(6, 1856, 1024, 0, "full perm_lds=0 red:table slab:lds cs:behind segs:above plain"),
    _row(6, 1856, 1024, 1, "full perm_lds=0 red:table slab:lds cs:behind segs:above plain-stream"),
]


def problem(case):
    """The row's image and start: X (n, p) counts, W0, H0, p."""
    k, n, p = case["k"], case["n_pad"], 2 * case["pb"] + 37
    rng = np.random.default_rng(9000 + n + k)
    Ht = rng.random((k, p)) ** 2 + 0.03
    Ht /= Ht.sum(axis=0, keepdims=True)
    Wt = rng.random((n, k)) ** 3 + 0.02
    Wt *= max(0.03, 4.0 / n) / (Wt @ Ht).mean()          # a few counts per pixel whatever n: ones, larger counts and padding in the lists
    X = np.minimum(rng.poisson(Wt @ Ht), 255).astype(np.float32)
    X[X.sum(axis=1) == 0, 0] = 1.0                       # (no empty line: their fill numerators would take the launch off the row's instance)
    X[0, X.sum(axis=0) == 0] = 1.0
    W0 = (rng.random((n, k)) * Wt.mean() * 2 + 1e-3).astype(np.float32)
    H0 = rng.random((k, p)) + 0.05
    return X, W0, (H0 / H0.sum(axis=0, keepdims=True)).astype(np.float32), p
