"""Every shape of the sparse store's fused launch plan on the device (tests/ell_plan_cases.py; csrc/mu_ell_plan.hpp): the fused launch
against the two launches, and the chained H-only launch (ESPM_H_CHAIN=1) against the general H-only path, with the tolerances
tests/test_gpu_estimator.py::test_sparse_store_mid_size_tiles holds the two paths to.  That each row reaches the shape it names is
tests/test_ell_plan_cpu.py's; here the engine's state is held to the row's arguments (n_pad, block size, streaming, no fill pixels,
no heavy elements), which is all the plan reads.  Three iterations with the loss: the first fused launch has no previous H (the
generic instance whatever the row), the second and third are the row's."""
import ctypes as C

import numpy as np
import pytest
import torch

import ell_plan_cases as ec

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5   # (tests/test_gpu_estimator.py)
ITERS = 3
KW = dict(simplex_H=True, simplex_W=False, lambda_L=0.7, mu=0.05)


def _engine(case, X, p, fused):
    from espm_amd.engine import MUEngine
    eng = MUEngine(X, case["k"], shape_2d=(1, p), x_store="ell", tile_px=case["pb"] // 2, fused=fused, tol=0.0, max_iter=ITERS + 2, **KW)
    st = eng.st
    assert eng.x_store == "ell" and (st.n_pad, st.ell_pb, st.nblk_w, st.ell_stream) == (case["n_pad"], case["pb"], 3, case["stream"])
    assert st.ell_fill_n == 0 and st.ell_hv_n == 0 and st.h_rule == 0
    assert eng.lib.espm_mu_fused_applies(C.byref(st)) == int(fused == "always")
    return eng


@pytest.mark.parametrize("case", ec.CASES, ids=[c["id"] for c in ec.CASES])
def test_fused_against_two_launches_and_chained_against_general(case, monkeypatch):
    monkeypatch.setenv("ESPM_ELL_STREAM_MB", "0" if case["stream"] else "1000000")
    for name in ("ESPM_FUSED", "ESPM_H_CHAIN", "ESPM_FORCE_ELL_TILE", "ESPM_ELL_KEEP_GROUPS", "ESPM_ELL_KEEP_MB", "ESPM_FUSED_PLAIN", "ESPM_FUSED_SMALL_SEGS"):
        monkeypatch.delenv(name, raising=False)
    X, W0, H0, p = ec.problem(case)
    out = {}
    for fused in ("always", False):
        eng = _engine(case, X, p, fused)
        eng.load_state(W0, H0)
        eng.iterate(ITERS, final_loss=True)
        torch.cuda.synchronize()
        out[fused] = (eng.history(), eng.get_H(), eng.get_W())
    (h, H, W), (ref_h, ref_H, ref_W) = out["always"], out[False]
    assert np.isfinite(h["loss"]).all() and len(h["loss"]) > ITERS and h["bad"].sum() == 0 and ref_h["bad"].sum() == 0
    np.testing.assert_allclose(h["loss"][1:], ref_h["loss"][1:], rtol=LOSS_RTOL)
    np.testing.assert_allclose(h["rel_W"][1:], ref_h["rel_W"][1:], rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(h["rel_H"][1:], ref_h["rel_H"][1:], rtol=2e-3, atol=1e-5)
    np.testing.assert_allclose(H, ref_H, rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(W, ref_W, rtol=2e-4, atol=2e-4 * np.abs(ref_W).mean())

    # H-only iterations on the engine of the two launches: the general path, then the chained launch from the same state
    alt = eng.hpart_alt.data_ptr()
    runs = []
    for chained in (False, True):
        eng.st.hpart_alt = alt if chained else None
        assert eng.h_chain_applies() == chained
        eng.load_state(W0, H0)
        eng.iterate_h(ITERS, final_loss=True)
        torch.cuda.synchronize()
        runs.append((eng.history(), eng.get_H()))
    (ref_h, ref_H), (h, H) = runs
    assert np.isfinite(h["loss"]).all() and len(h["loss"]) > ITERS
    np.testing.assert_allclose(h["loss"][1:], ref_h["loss"][1:], rtol=LOSS_RTOL)
    np.testing.assert_allclose(h["rel_H"][1:], ref_h["rel_H"][1:], rtol=2e-3, atol=1e-5)
    np.testing.assert_allclose(H, ref_H, rtol=2e-4, atol=2e-5)
