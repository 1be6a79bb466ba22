"""transform() without a GPU: the yardstick of tests/test_gpu_transform.py and the declarations of its C entry points.

The H that ``transform`` returns is defined by the reference's own fit with every entry of W imposed (fixed_W = W, updates.py:75-76);
the tests compare with ``oracle.mu_oracle.fit(..., W=Wf, fixed_W=Wf)``, which fixtures F6 and F21 pin to the reference.  Here: that call
is what it is taken for - W does not move, rel_W is 0, and the trajectory is the H rule alone under the reference's stop rules."""
import os
import re

import numpy as np
import pytest

from oracle import mu_oracle as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(seed=0, n=40, nx=12, ny=10, k=3):
    rng = np.random.default_rng(seed)
    W = rng.random((n, k)) + 0.05
    H = rng.random((k, nx * ny)) + 0.05
    H /= H.sum(axis=0, keepdims=True)
    X = rng.poisson(40.0 * (W @ H)).astype(np.float64)
    Wf = W * (1.0 + 0.1 * rng.standard_normal(W.shape)).clip(0.5, 1.5)
    Wf[3, 1] = oc.LOG_SHIFT   # (an entry on the floor of initialize_algorithms, where a fit's W_ may sit)
    return X, Wf, rng


@pytest.mark.parametrize("flat_h", [False, True], ids=["supplied_H", "flat_H"])
def test_oracle_with_every_entry_of_w_fixed_is_an_h_only_fit(flat_h):
    X, Wf, rng = _problem()
    k, (nx, ny) = 3, (12, 10)
    p = nx * ny
    H0 = np.full((k, p), 1.0 / k) if flat_h else (lambda h: h / h.sum(axis=0, keepdims=True))(rng.random((k, p)) + 0.1)
    kw = dict(lambda_L=1.0, mu=0.1, simplex_H=True, simplex_W=False, shape_2d=(nx, ny), tol=1e-4, max_iter=200)
    ref = oc.fit(X, k, W=Wf.copy(), H=H0.copy(), fixed_W=Wf.copy(), **kw)
    # W stays exactly where it was, rel_W = 0 on every iteration
    np.testing.assert_array_equal(ref["W"], np.maximum(Wf, oc.LOG_SHIFT))
    assert np.all(ref["rel"][:, 0] == 0.0)
    assert ref["exit"] == "loss" and 2 <= ref["n_iter"] < 200

    # the same trajectory by hand: multiplicative_step_h and the stop rules (base.py:313-394), iteration for iteration
    X_ = oc.remove_zeros_lines(X, oc.LOG_SHIFT)
    W_, H_ = np.maximum(Wf, oc.LOG_SHIFT), np.maximum(H0, oc.LOG_SHIFT)
    G_ = np.eye(X.shape[0])
    L_ = oc.laplacian_matrix(nx, ny)
    c_kl = oc.const_KL(X_, oc.LOG_SHIFT)

    def loss(H):
        return oc.smooth_nmf_loss(X_, G_, W_, H, L_, 0.1, 1, 1.0, oc.LOG_SHIFT, True, c_kl, oc.SIGMA_L)[0]

    eval_init, eval_before = loss(H_), np.inf
    losses, rel_h, reason = [], [], None
    while True:
        old = H_.copy()
        H_ = oc.multiplicative_step_h(X_, G_, W_, H_, simplex_H=True, mu=0.1, log_shift=oc.LOG_SHIFT, epsilon_reg=1, safe=False,
                                      dicotomy_tol=oc.DICOTOMY_TOL, lambda_L=1.0, L=L_, sigmaL=oc.SIGMA_L)
        losses.append(loss(H_))
        rel_h.append(np.max(np.abs(H_ - old) / (H_ + 1e-4 * np.mean(H_))))
        if len(losses) >= 200:
            reason = "max_iter"
        elif rel_h[-1] < 1e-4:
            reason = "rel"
        elif abs((eval_before - losses[-1]) / eval_init) < 1e-4:
            reason = "loss"
        elif eval_before - losses[-1] < 0:
            reason = "increase"
        if reason:
            break
        eval_before = losses[-1]
    assert (len(losses), reason) == (ref["n_iter"], ref["exit"])
    np.testing.assert_array_equal(np.array(losses), ref["losses"])
    np.testing.assert_array_equal(np.array(rel_h), ref["rel"][:, 1])
    np.testing.assert_array_equal(H_, ref["H"])


def _declarations(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {name: " ".join(m.split()) for name in ("espm_mu_iterate_h", "espm_mu_h_chain_applies")
            for m in re.findall(r"int\s+%s\s*\([^)]*\)\s*;" % name, text)}


def test_header_and_packaged_copy_declare_the_h_only_entry_points():
    with open(os.path.join(ROOT, "include", "espm_mu.h")) as f:
        ours = _declarations(f.read())
    assert ours == {"espm_mu_iterate_h": "int espm_mu_iterate_h(espm_mu_state* st, int n_iter, int final_loss, espm_stream_t stream);",
                    "espm_mu_h_chain_applies": "int espm_mu_h_chain_applies(const espm_mu_state* st);"}
    packaged = os.path.join(ROOT, "espm_amd", "include", "espm_mu.h")   # (placed next to the library by the build)
    assert os.path.exists(packaged), "the package carries no copy of include/espm_mu.h: run the build"
    with open(packaged) as f:
        assert _declarations(f.read()) == ours
    # ... and the binding knows both, with the header's arguments
    import ctypes as C
    from espm_amd import _lib
    assert _lib.SYMBOLS["espm_mu_iterate_h"][0] is C.c_int and len(_lib.SYMBOLS["espm_mu_iterate_h"][1]) == 4
    assert _lib.SYMBOLS["espm_mu_h_chain_applies"][0] is C.c_int and len(_lib.SYMBOLS["espm_mu_h_chain_applies"][1]) == 1
    assert hasattr(_lib.lib, "espm_mu_iterate_h") and hasattr(_lib.lib, "espm_mu_h_chain_applies")
