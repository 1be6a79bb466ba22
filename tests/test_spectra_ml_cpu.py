"""The spectra ML without a device: what the GPU tests (test_gpu_spectra_ml.py) rest on, held by the numpy restatement alone
(tests/spectra_ml_reference.py) - the identities of the pass's sums, the certificate at every accepted point, the condition that
every fit of every case converges within half of MAX_PASS, what the statistic says on planted entries - and the argument errors of
``spectra_ml.ml_spectra``, ``spectra_ml.presence`` and ``est.element_presence`` before any upload."""
import numpy as np
import pytest

import spectra_ml_reference as R

TOL = 1e-3
CHI2_95 = 2.71   # the 95 % point of the boundary mixture 1/2 chi2_0 + 1/2 chi2_1 (the 90 % point of chi2_1: 2.7055)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


# ---- the sums of the pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_ratio_sums_return_the_counts(name):
    """sum_j d_cj q_cj = sum_p (x / y) (d_c . h_p) = sum_p x on every channel without a floored entry: y IS d_c . h_p there.  Both
    sides are sums of p + k non-negative terms: C4 (p + k + 2) eps relative, the bound of q."""
    X, G, W, H = R.case(name)
    p, k = X.shape[1], H.shape[0]
    D = G @ W
    s = R.sums(X, D, H)
    ok = ~s["floored"]
    assert 0 < (~ok).sum() < ok.size and s["unmodelled"] == 1   # (the zero row of G, and the one count in it)
    lhs = (D * s["Q"]).sum(axis=1)
    err = np.abs(lhs - s["xsum"])[ok]
    print(f"{name}: worst {np.max(err / np.maximum(s['xsum'][ok], 1)):.3g} relative")
    assert (err <= R.C4 * (p + k + 2) * R.EPS * s["xsum"][ok]).all()


def test_A_is_minus_the_derivative_of_q():
    """dq_cj / dd_ci = -sum_p x h_j h_i / y^2 = -A_c,ij, by central differences in d (relative step 1e-5: truncation ~1e-10 relative,
    rounding ~1e-11; held to 1e-7 of the largest entry of the channel's A)."""
    X, G, W, H = R.case("k3")
    D = G @ W
    s = R.sums(X, D, H)
    ok = ~s["floored"]
    for i in range(3):
        step = 1e-5 * D[:, i]
        up, dn = np.array(D), np.array(D)
        up[:, i] += step
        dn[:, i] -= step
        dq = (R.sums(X, up, H)["Q"] - R.sums(X, dn, H)["Q"])[ok] / (2.0 * step[ok, None])
        scale = np.abs(s["A"][ok]).max(axis=(1, 2))[:, None]
        assert (np.abs(dq + s["A"][ok][:, :, i]) <= 1e-7 * scale).all()
    assert np.array_equal(s["A"], s["A"].transpose(0, 2, 1))


def test_the_em_successor_is_the_unregularised_w_step():
    """e = W o r is the multiplicative update W o (G^T (X / (G W H)) H^T) / (G^T 1 1^T H^T), written out."""
    X, G, W, H = R.case("k5")
    x = X.astype(np.float64)
    Y = np.maximum(G @ W @ H, R.LOG_SHIFT)
    step = W * (G.T @ (x / Y) @ H.T) / (G.T @ np.ones_like(x) @ H.T)
    ev = R.evaluate(X, G, H, W)
    np.testing.assert_allclose(W * ev["r"], step, rtol=1e-12)
    # ... and it does not raise the deviance
    assert R.evaluate(X, G, H, step)["deviance"] <= ev["deviance"]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASES)
def test_certificate_at_every_accepted_point(name):
    """dev - dev_opt <= the certificate's bound at every accepted point, to 1e-9 max(1, dev) as test_pixel_ml_pinned_cpu.py holds its
    rule.  The bound is ``gap`` wherever no counted entry sits under the floor; every case here has one (3 counts in the zero row of
    G), and there it is 2 U + max(gap, 0) (the reference's docstring derives it).  The accepted deviances never increase."""
    X, G, _, H = R.case(name)
    sol, opt = R.solved(name), R.optimum(name)
    assert sol["converged"] and len(sol["accepted"]) == sol["n_pass"] - sol["n_rejected"]
    last = np.inf
    for W, dev, gap, _ in sol["accepted"]:
        ev = R.evaluate(X, G, H, W)
        assert ev["certificate_slack"] == 6.0 and abs(ev["gap"] - gap) <= 1e-6 * max(1.0, abs(gap))
        assert dev - opt["deviance"] <= R.certificate_bound(gap, ev["certificate_slack"]) + 1e-9 * max(1.0, dev)
        assert dev >= opt["deviance"] - opt["gap"] - 1e-9 * max(1.0, dev) and dev <= last
        last = dev
    print(f"{name}: {sol['n_pass']} passes, dev - dev_opt = {sol['deviance'] - opt['deviance']:.3g}, gap {sol['gap']:.3g}")
    assert sol["deviance"] <= opt["deviance"] + TOL


def test_certificate_without_a_count_under_the_floor():
    """The same images with the one floored count taken out: U = 0, and dev - dev_opt <= gap itself at every accepted point.  The
    optimum is a long EM run, certified by its own rigorous gap."""
    for name in ("k3", "k8", "k1"):
        X, G, _, H = R.case(name)
        X = np.array(X)
        X[~((G.sum(axis=1) > 0))] = 0
        sol = R.ml_spectra(X, G, H, tol=TOL, history=True)
        opt = R.em(X, G, H, n_iter=40000)
        F, _ = R.free_set(G, H)
        ev_opt = R.evaluate(X, G, H, opt["W"])
        room = R.rigorous_gap(ev_opt, opt["W"], F)
        assert sol["converged"] and sol["unmodelled"] == 0 and 0 <= room <= 1e-6
        for W, dev, gap, un in sol["accepted"]:
            assert un == 0 and dev - ev_opt["deviance"] <= gap + 1e-9 * max(1.0, dev)
        assert -1e-6 <= sol["gap"] <= TOL and sol["deviance"] <= ev_opt["deviance"] + TOL
        print(f"{name}: {sol['n_pass']} passes, final gap {sol['gap']:.3g}, dev - dev_opt = {sol['deviance'] - ev_opt['deviance']:.3g}")


@pytest.mark.parametrize("name", R.CASES)
def test_every_fit_converges_within_half_the_cap(name):
    """THE CONDITION the GPU tests rest on: the full fit and every nested fit of every case converge within MAX_PASS // 2."""
    full, nested = R.solved(name), R.tested(name)
    print(f"{name}: full fit {full['n_pass']} passes ({full['n_rejected']} rejected, {full['n_fallback']} fallbacks), nested at most "
          f"{nested['n_pass'][1:].max()}")
    assert R.MAX_PASS == 64 and full["converged"] and full["n_pass"] <= R.MAX_PASS // 2
    assert nested["converged"].all() and nested["n_pass"].max() <= R.MAX_PASS // 2 and (nested["gap"] <= TOL).all()
    assert not np.isnan(nested["lr"]).any() and (nested["lr"] >= 0).all()


def test_planted_entries():
    """Entries of W planted at zero have lr below the 95 % point of the mixture; the ten largest true entries lie far above it."""
    _, _, W, _ = R.case("planted")
    lr = R.tested("planted")["lr"]
    absent = [lr[e, j] for e, j in R.PLANTED_AT]
    top = np.argsort(W.ravel())[-10:]
    print(f"planted absent: lr {absent}; the ten largest true entries: lr {lr.ravel()[top].min():.3g} .. {lr.ravel()[top].max():.3g}")
    assert all(W[e, j] == 0 for e, j in R.PLANTED_AT) and max(absent) < CHI2_95
    assert (lr.ravel()[top] > CHI2_95).all()
    pv = R.tested("planted")["pvalue"]
    assert all(pv[e, j] > 0.05 for e, j in R.PLANTED_AT) and (pv.ravel()[top] < 0.05).all()


def test_free_inert_and_an_image_without_counts():
    X, G, _, H = R.case("k3")
    free = np.ones((6, 3), dtype=bool)
    free[2, 1] = free[5, 0] = False
    sub, full = R.ml_spectra(X, G, H, free=free), R.solved("k3")
    assert sub["converged"] and sub["W"][2, 1] == 0 and sub["W"][5, 0] == 0 and (sub["W"][free] > 0).all()
    assert sub["deviance"] >= full["deviance"] - TOL   # a smaller feasible set
    np.testing.assert_allclose(R.column_sums(G, H)[free] @ sub["W"][free], X.sum(), rtol=1e-14)
    Gz = np.array(G)
    Gz[:, 4] = 0.0
    got = R.ml_spectra(X, Gz, H)
    assert got["converged"] and got["inert"][4].all() and got["inert"].sum() == 3 and not got["W"][4].any()
    none = R.ml_spectra(np.zeros_like(X), G, H)
    assert none["converged"] and none["n_pass"] == 0 and not none["W"].any() and none["deviance"] == 0 and none["gap"] == 0
    with pytest.raises(ValueError, match="no free entry"):
        R.ml_spectra(X, G, H, free=np.zeros((6, 3), dtype=bool))
    # an entry that is not tested, and one outside the free set, stay NaN
    part = R.presence(X, G, H, free=free, entries=[[0, 0], [2, 1]])
    assert np.isnan(part["lr"]).sum() == 17 and part["lr"][0, 0] >= 0 and part["n_pass"][2] == 0


# ---- the binding and the refusals before any upload -----------------------------------------------------------------------------------------
def test_binding_and_refusals_before_any_launch(lib):
    import ctypes as C
    f = lib.lib.espm_spectra_ml_pass
    assert f.restype is C.c_int and len(f.argtypes) == 19 and lib.lib.espm_spectra_ml_pass_scratch.restype is C.c_size_t
    assert lib.lib.espm_spectra_ml_pass_scratch(300, 2125, 5) == 2 * (3 + 5 + 15) * 300 * 8
    assert lib.lib.espm_spectra_ml_pass_scratch(300, 2125, 9) == 0
    buf = (C.c_double * 4096)()
    ptr = C.cast(buf, C.c_void_p)
    args = lambda k=2, shift=1e-14, nbytes=1 << 20, x=ptr, ld=10: (x, lib.DIAG_X_F64, lib.LAYOUT_CM, ld, 4, 10, ptr, ptr, k, shift, ptr, ptr,  # noqa: E731
                                                                   ptr, ptr, ptr, ptr, ptr, nbytes, None)
    for bad, code, text in ((dict(k=9), lib.EUNSUPPORTED, "k=9"), (dict(k=0), lib.EUNSUPPORTED, "k=0"), (dict(x=None), lib.EINVAL, "bad arguments"),
                            (dict(shift=0.0), lib.EINVAL, "log_shift must be positive"), (dict(ld=9), lib.EINVAL, "ld=9"),
                            (dict(nbytes=8), lib.EINVAL, "scratch of 8 bytes")):
        assert f(*args(**bad)) == code and text in lib.last_error(), bad


def test_argument_errors_come_before_the_upload(lib, monkeypatch):
    from espm_amd import _image, spectra_ml
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X, G, H = np.zeros((6, 10), np.float32), np.ones((6, 4)), np.ones((2, 10))
    for fn in (spectra_ml.ml_spectra, spectra_ml.presence):
        with pytest.raises(NotImplementedError, match="G is required"):
            fn(X, None, H)
        with pytest.raises(NotImplementedError, match="9 components"):
            fn(X, G, np.ones((9, 10)))
        with pytest.raises(NotImplementedError, match="2052 rows"):
            fn(X, np.ones((6, 513)), np.ones((4, 10)))
        with pytest.raises(ValueError, match="channels"):
            fn(X, np.ones((5, 4)), H)
        with pytest.raises(ValueError, match="pixels"):
            fn(X, G, np.ones((2, 11)))
        with pytest.raises(ValueError, match="tol"):
            fn(X, G, H, tol=0.0)
        with pytest.raises(ValueError, match="log_shift"):
            fn(X, G, H, log_shift=0.0)
        with pytest.raises(ValueError, match="max_pass"):
            fn(X, G, H, max_pass=0)
        with pytest.raises(ValueError, match="layout"):
            fn(X, G, H, layout="xy")
        with pytest.raises(ValueError, match="not negative"):
            fn(X, -G, H)
        with pytest.raises(ValueError, match="W0 of shape"):
            fn(X, G, H, W0=np.ones((4, 3)))
        with pytest.raises(ValueError, match="not finite"):
            fn(X, G, H, W0=np.full((4, 2), np.nan))
        with pytest.raises(ValueError, match="free must be"):
            fn(X, G, H, free=np.ones((4, 2)))
        with pytest.raises(ValueError, match="no free entry"):
            fn(X, G, H, free=np.zeros((4, 2), dtype=bool))
        with pytest.raises(ValueError, match="not finite"):
            fn(np.full((6, 10), np.inf, np.float32), G, H)
    for ent in ([[4, 0]], [[0, 2]], [[0, 0], [0, 0]], [0, 1], [[0.5, 1.0]]):
        with pytest.raises(ValueError, match="entries"):
            spectra_ml.presence(X, G, H, entries=ent)
    assert spectra_ml.MAX_PASS == R.MAX_PASS == 64


def test_estimator_refuses_before_the_upload(lib, monkeypatch):
    from espm_amd import _image
    from espm_amd.estimators import SmoothNMF
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X = np.zeros((6, 10), np.float32)
    with pytest.raises(Exception, match="not fitted"):
        SmoothNMF(n_components=2).element_presence(X)

    def fitted(k, G, fixed_W=None):
        est = SmoothNMF(n_components=k, fixed_W=fixed_W)
        est.G_, est._identity_G = (np.eye(6), True) if G is None else (G, False)
        est.W_, est.H_ = np.ones((est.G_.shape[1], k)), np.ones((k, 10))
        return est
    G = np.ones((6, 4))
    with pytest.raises(NotImplementedError, match="9 components"):
        fitted(9, G).element_presence(X)
    with pytest.raises(NotImplementedError, match="dictionary or physics model"):
        fitted(2, None).element_presence(X)
    fixed = -np.ones((4, 2))
    fixed[1, 1], fixed[2, 0] = 0.0, 0.3
    held = fitted(2, G, fixed)
    with pytest.raises(NotImplementedError, match="positive"):
        held.element_presence(X)
    with pytest.raises(ValueError, match="channels"):
        fitted(2, G).element_presence(np.zeros((5, 10), np.float32))
    with pytest.raises(ValueError, match="entries"):
        fitted(2, G).element_presence(X, entries=[[9, 9]])
    assert not hasattr(held, "W_ml_")


def test_adapter_needs_the_analysis(lib):
    from espm_amd import hyperspy_adapter as ha
    from espm_amd.estimators import SmoothNMF
    with pytest.raises(AttributeError, match="element_presence"):
        ha.element_presence(SmoothNMF(n_components=2))
