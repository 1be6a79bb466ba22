"""Pixel ML and the presence maps on the device (csrc/mu_pixel_ml.hip, espm_amd/presence.py) against the rule restated in numpy
(tests/pixel_ml_reference.py).  The correctness checks are SOLVER-AGNOSTIC: the certificate is recomputed in numpy from the returned
h, in deviance units, with tolerances that follow from the certificate and fp64 rounding over n <= 300 terms.  What the kernel
promises bit for bit - both layouts, every dtype, every split into calls, padded rows, a slab - is compared with ``np.array_equal``.
test_pixel_ml_cpu.py holds the condition all of this rests on: the reference alone converges everywhere within half of MAX_PASS."""
import ctypes as C
import functools

import numpy as np
import pytest

import pixel_ml_reference as pr

pytestmark = pytest.mark.gpu

TOL = 1e-3
KEYS = ("H", "deviance", "gap", "n_pass", "converged")


@pytest.fixture(scope="module")
def presence():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import presence
    return presence


def _unmix(X, D, H0, layout="cm", **kw):
    from espm_amd import presence
    kw.setdefault("max_pass", pr.MAX_PASS)
    return presence.ml_unmix(X, D, H0, tol=kw.pop("tol", TOL), layout=layout, **kw)


@functools.lru_cache(maxsize=None)
def _solved(name):
    """The device's fit of a named case from the reference's start (shared: read-only)."""
    X, D = pr.case(name)
    return _unmix(X, D, pr.start_from(X, D))


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys) and a["unmodelled"] == b["unmodelled"]


# ---- solver-agnostic correctness ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.CASES)
def test_certificate_recomputed_in_numpy(presence, name):
    X, D = pr.case(name)
    got, opt = _solved(name), pr.optimum(name)
    assert got["converged"].all() and got["nonfinite"] == 0 and got["unmodelled"] == 0
    assert got["H"].shape == (D.shape[1], X.shape[1]) and got["n_pass"].dtype.kind == "i" and got["converged"].dtype == bool
    ev = pr.evaluate(X, D, got["H"])
    dev, N = got["deviance"], ev["N"]
    scale = np.maximum(1.0, dev)
    print(f"{name}: passes <= {got['n_pass'].max()}, gap_numpy - tol <= {np.max(ev['gap'] - TOL):.3g}, "
          f"|dev - dev_numpy| / scale <= {np.max(np.abs(dev - ev['deviance']) / scale):.3g}, dev - dev_opt in "
          f"[{np.min(dev - opt['deviance']):.3g}, {np.max(dev - opt['deviance']):.3g}]")
    assert (ev["gap"] <= TOL * (1 + 1e-9) + 1e-12 * N).all()
    assert (got["gap"] <= TOL).all()
    assert (np.abs(dev - ev["deviance"]) <= 1e-10 * scale).all()
    assert (dev >= opt["deviance"] - 1e-9 * scale).all() and (dev <= opt["deviance"] + TOL).all()
    live = N > 0
    np.testing.assert_allclose((D.sum(axis=0) @ got["H"])[live], N[live], rtol=1e-14)   # h as scaled in step 1
    assert (got["H"] >= 0).all()


@pytest.mark.parametrize("name", pr.CASES)
def test_agreement_with_the_references_trajectory(presence, name):
    """The same start, the same rule: the pass counts are those of the reference but for pixels within rounding of the threshold (at
    most 1 %, one pass apart), and the deviances agree within what the two certificates allow (both within ``gap`` <= tol of one
    minimum) - a bound on the deviance, not on h."""
    got, ref = _solved(name), pr.solved(name)
    differ = got["n_pass"] != ref["n_pass"]
    print(f"{name}: {differ.sum()} of {differ.size} pixels stop a pass apart; |dev - dev_ref| <= {np.max(np.abs(got['deviance'] - ref['deviance'])):.3g}")
    assert differ.mean() <= 0.01 and (np.abs(got["n_pass"] - ref["n_pass"]) <= 1).all()
    scale = np.maximum(1.0, ref["deviance"])
    assert (np.abs(got["deviance"] - ref["deviance"]) <= TOL + 1e-9 * scale).all()
    same = ~differ
    assert np.allclose(got["H"][:, same], ref["H"][:, same], rtol=1e-6, atol=1e-9 * ref["N"].max())   # the same trajectory, pass for pass


# ---- what is promised bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["img96_k3", "planted", "tall"])
def test_both_layouts_and_every_dtype_give_the_same_bits(presence, name):
    X, D = pr.case(name)
    H0, want = pr.start_from(X, D), _solved(name)
    assert _same(_unmix(np.ascontiguousarray(X.T), D, H0, layout="pm"), want)
    for dtype in (np.uint16, np.float32, np.float64):
        assert _same(_unmix(X.astype(dtype), D, H0), want), dtype
        assert _same(_unmix(np.ascontiguousarray(X.T).astype(dtype), D, H0, layout="pm"), want), dtype


@pytest.mark.parametrize("name", ["img96_k3", "tall"])
def test_the_split_into_calls_does_not_matter(presence, name):
    X, D = pr.case(name)
    H0, want = pr.start_from(X, D), _solved(name)
    assert want["n_pass"].max() > 64   # (more than one default chunk)
    for chunk in (1, 7, pr.MAX_PASS):
        assert _same(_unmix(X, D, H0, chunk=chunk), want), chunk


def test_padded_rows_and_a_slab(presence):
    import torch
    X, D = pr.case("img96_k3")
    H0, want = pr.start_from(X, D), _solved("img96_k3")
    for layout, Xl in (("cm", X), ("pm", np.ascontiguousarray(X.T))):
        wide = torch.zeros((Xl.shape[0], Xl.shape[1] + 13), dtype=torch.uint8, device="cuda")
        wide[:, :Xl.shape[1]] = torch.from_numpy(Xl).cuda()
        view = wide[:, :Xl.shape[1]]
        assert view.stride(0) == Xl.shape[1] + 13
        assert _same(_unmix(view, D, H0, layout=layout), want), layout
    # the pixels 256 .. 1320 alone, as a copy and as a view into the whole image on the device (ld = 1320, an odd first address)
    part = _unmix(np.ascontiguousarray(X[:, 256:]), D, H0[:, 256:])
    assert all(np.array_equal(part[k], want[k][..., 256:]) for k in KEYS)
    whole = torch.from_numpy(np.array(X)).cuda()
    assert all(np.array_equal(_unmix(whole[:, 257:], D, H0[:, 257:])[k], want[k][..., 257:]) for k in KEYS)
    pm = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    assert all(np.array_equal(_unmix(pm[256:], D, H0[:, 256:], layout="pm")[k], want[k][..., 256:]) for k in KEYS)


# ---- the state rules, through the entry point itself --------------------------------------------------------------------------------------
class _Raw:
    """The entry point on device tensors of the caller: the state is in plain sight."""

    def __init__(self, name, mask=None, H0=None):
        import torch
        X, D = pr.case(name)
        self.n, self.p, self.k = X.shape[0], X.shape[1], D.shape[1]
        self.mask = (1 << self.k) - 1 if mask is None else mask
        self.s = np.ascontiguousarray(D.sum(axis=0))
        self.X, self.D = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(D)).cuda()
        self.H = torch.from_numpy(np.ascontiguousarray(pr.start_from(X, D) if H0 is None else H0)).cuda()
        self.dev, self.gap = (torch.full((self.p,), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
        self.passes = torch.zeros(self.p, dtype=torch.int32, device="cuda")
        self.done = torch.zeros(self.p, dtype=torch.uint8, device="cuda")
        self.counters = torch.zeros(3, dtype=torch.int64, device="cuda")

    def call(self, n_pass, tol=TOL):
        from espm_amd import _lib
        from espm_amd.engine import _ptr, _stream
        rc = _lib.lib.espm_pixel_ml(_ptr(self.X), _lib.DIAG_X_U8, _lib.LAYOUT_CM, self.p, self.n, self.p, _ptr(self.D),
                                    self.s.ctypes.data_as(C.c_void_p), self.k, self.mask, 1e-14, tol, n_pass, _ptr(self.H), _ptr(self.dev),
                                    _ptr(self.gap), _ptr(self.passes), _ptr(self.done), _ptr(self.counters), _stream())
        _lib.check(rc)
        return self

    def state(self):
        return tuple(t.cpu().numpy().copy() for t in (self.H, self.dev, self.gap, self.passes, self.done, self.counters))


def test_resumable_and_a_done_pixel_is_never_touched(presence):
    one = _Raw("planted").call(90).state()
    two = _Raw("planted").call(20)
    mid = two.state()
    then = two.call(70).state()
    assert all(np.array_equal(a, b) for a, b in zip(one, then))   # 20 + 70 passes: the bits of 90, counters included
    done_mid = mid[4] == 1
    assert 0 < done_mid.sum() < done_mid.size and 0 < (then[4] == 1).sum() < done_mid.size   # (some done after 20, not all after 90)
    assert then[5][0] == (then[4] == 0).sum() and mid[5][0] == (mid[4] == 0).sum()           # the one integer the host loop reads
    for a, b in zip(mid[:5], then[:5]):
        assert np.array_equal(a[..., done_mid], b[..., done_mid])
    assert (then[3][then[4] == 0] == 90).all() and (then[2][then[4] == 0] > TOL).all() and (then[2][then[4] == 1] <= TOL).all()
    # all done: a further call writes nothing at all
    full = _Raw("img96_k2").call(pr.MAX_PASS)
    before = full.state()
    assert before[5][0] == 0 and (before[4] == 1).all()
    full.H += 1.0   # (were a done pixel rewritten, its h would come back scaled)
    after = full.call(50).state()
    assert np.array_equal(after[0], before[0] + 1.0) and all(np.array_equal(a, b) for a, b in zip(before[1:], after[1:]))


def test_empty_pixels_masked_rows_and_starts_that_are_not_positive(presence):
    X, D = pr.case("planted")
    got = _solved("planted")
    assert not X[:, 5].any()
    assert not got["H"][:, 5].any() and got["deviance"][5] == 0 and got["gap"][5] == 0 and got["n_pass"][5] == 0 and got["converged"][5]
    # a component set: the rows outside it are exactly 0 whatever the start holds there
    H0 = pr.start_from(X, D)
    sub = _unmix(X, D, H0, components=[0, 2])
    ref = pr.ml_unmix(X, D, H0, [0, 2], TOL, pr.MAX_PASS)
    assert not sub["H"][[1, 3]].any() and sub["converged"].all()
    assert (np.abs(sub["n_pass"] - ref["n_pass"]) <= 1).all() and (sub["n_pass"] != ref["n_pass"]).mean() <= 0.01
    assert (np.abs(sub["deviance"] - ref["deviance"]) <= TOL + 1e-9 * np.maximum(1.0, ref["deviance"])).all()
    # entries of the start that are not > 0 (zero, negative) become N / (|M| s_j) * 1e-3: the same bits as that start given outright
    N, s = X.sum(axis=0).astype(np.float64), D.sum(axis=0)
    holes = H0.copy()
    holes[0, ::3], holes[2, 1::4], holes[1] = 0.0, -1.0, 5.0
    filled = holes.copy()
    for j in (0, 2):
        bad = ~(holes[j] > 0)
        filled[j, bad] = (N / (2.0 * s[j]) * 1e-3)[bad]
    assert _same(_unmix(X, D, holes, components=[0, 2]), _unmix(X, D, filled, components=[0, 2]))
    # no start at all: N / sum_M s, the reference's default
    auto, want = _unmix(X, D, None), pr.ml_unmix(X, D, None, None, TOL, pr.MAX_PASS)
    assert auto["converged"].all() and (np.abs(auto["n_pass"] - want["n_pass"]) <= 1).all()
    assert (auto["n_pass"] != want["n_pass"]).mean() <= 0.01


def test_an_all_zero_spectrum_inside_and_outside_the_set(presence):
    X, D = pr.case("planted")
    Dz = np.array(D)
    Dz[:, 1] = 0.0
    with pytest.raises(ValueError, match="component 1"):
        _unmix(X, Dz, None)
    raw = _Raw("planted")
    raw.s[1] = 0.0
    with pytest.raises(ValueError, match="component 1"):
        raw.call(1)
    out = _unmix(X, Dz, pr.start_from(X, Dz), components=[0, 2, 3])
    assert out["converged"].all() and not out["H"][1].any()
    ev = pr.evaluate(X, Dz, out["H"], pr.mask_of(4, [0, 2, 3]))
    assert (ev["gap"] <= TOL * (1 + 1e-9) + 1e-12 * ev["N"]).all()


# ---- the counters -------------------------------------------------------------------------------------------------------------------------
def test_unmodelled_counts_the_planted_entries(presence):
    """A channel no spectrum reaches, with counts planted in it: every such entry sits under the floor and is counted once."""
    X, D = pr.case("planted")
    Dz, Xz = np.array(D), np.array(X)
    Dz[7] = 0.0
    Xz[7] = 0
    Xz[7, [3, 5, 40, 299]] = (1, 2, 1, 9)   # (pixel 5 holds no other count: N = 2, every spectrum misses its one channel)
    out = _unmix(Xz, Dz, pr.start_from(Xz, Dz))
    ref = pr.ml_unmix(Xz, Dz, pr.start_from(Xz, Dz), None, TOL, pr.MAX_PASS)
    assert out["converged"].all() and out["unmodelled"] == 4 == ref["unmodelled"] and out["nonfinite"] == 0
    assert _same(_unmix(np.ascontiguousarray(Xz.T), Dz, pr.start_from(Xz, Dz), layout="pm"), out)


def test_a_cap_too_small_leaves_the_pixels_the_reference_leaves(presence):
    X, D = pr.case("planted")
    H0 = pr.start_from(X, D)
    out, ref = _unmix(X, D, H0, max_pass=50), pr.ml_unmix(X, D, H0, None, TOL, 50)
    left = ~out["converged"]
    assert 0 < left.sum() < left.size and np.array_equal(out["converged"], ref["converged"])
    assert (out["gap"][left] > TOL).all() and (out["n_pass"][left] == 50).all() and (out["n_pass"][~left] < 50).all()
    assert np.allclose(out["gap"][left], ref["gap"][left], rtol=1e-6) and np.allclose(out["H"], ref["H"], rtol=1e-6, atol=1e-12)
    assert _same(_unmix(X, D, H0, max_pass=50, chunk=7), out)


# ---- presence -----------------------------------------------------------------------------------------------------------------------------
def test_presence_on_the_planted_image(presence):
    X, D, H, gone = pr.planted()
    out = presence.presence(X, D, tol=TOL, max_pass=pr.MAX_PASS)
    ref = pr.presence(X, D, None, TOL, pr.MAX_PASS)
    k, p = H.shape
    assert out["lr"].shape == out["pvalue"].shape == (k, p) and out["converged"].shape == out["gap"].shape == out["n_pass"].shape == (k + 1, p)
    assert out["converged"].all() and (out["gap"] <= TOL).all()
    assert (out["lr"] >= 0).all() and (out["pvalue"][out["lr"] == 0] == 1.0).all() and ((out["pvalue"] > 0) & (out["pvalue"] <= 1)).all()
    assert np.array_equal(out["pvalue"], pr.pvalue(out["lr"]))
    assert (np.abs(out["lr"] - ref["lr"]) <= 2 * TOL + 1e-9 * np.maximum(1.0, ref["deviance_ml"])[None, :]).all()   # two certified deviances each
    carried = H * D.sum(axis=0)[:, None]
    for j in range(k):
        absent, strong = np.median(out["pvalue"][j][gone[j]]), np.median(out["pvalue"][j][carried[j] >= 20])
        print(f"component {j}: median p {absent:.3g} where planted absent ({gone[j].sum()} pixels), {strong:.3g} where it carries >= 20 counts "
              f"({(carried[j] >= 20).sum()} pixels)")
        assert absent > 0.25 and strong < 1e-3
    full = _unmix(X, D, None)
    assert np.array_equal(out["H_ml"], full["H"]) and np.array_equal(out["deviance_ml"], full["deviance"])


def test_presence_with_one_component_takes_the_host_path(presence, monkeypatch):
    X, D = pr.case("img96_k1")
    runs = []
    real = presence._Solver.run
    monkeypatch.setattr(presence._Solver, "run", lambda self, *a: runs.append(a[2]) or real(self, *a))
    out, ref = presence.presence(X, D), pr.presence(X, D)
    assert runs == [1]   # the full fit alone was launched
    assert out["lr"].shape == (1, X.shape[1]) and out["converged"].all() and not out["n_pass"][1].any()
    assert np.allclose(out["lr"], ref["lr"], rtol=1e-12) and (out["lr"] > 0).all()
    assert _same(dict(out, H=out["H_ml"], deviance=out["deviance_ml"], gap=out["gap"][0], n_pass=out["n_pass"][0], converged=out["converged"][0]),
                 _unmix(X, D, None))


# ---- the estimator and the adapter --------------------------------------------------------------------------------------------------------
SHAPE = (15, 20)


def _fit(simplex_H=False, hspy_comp=False):
    from espm_amd.estimators import SmoothNMF
    X = pr.case("planted")[0]
    est = SmoothNMF(n_components=3, max_iter=200, tol=0.0, verbose=0, random_state=0, shape_2d=SHAPE, simplex_H=simplex_H, simplex_W=not simplex_H, hspy_comp=hspy_comp)
    Xin = np.ascontiguousarray(X.T) if hspy_comp else X
    est.fit(Xin.astype(np.float32))
    return est, Xin


@pytest.mark.parametrize("hspy_comp", [False, True], ids=["cm", "hspy"])
def test_estimator_and_adapter(presence, hspy_comp):
    from espm_amd import hyperspy_adapter as ha
    est, Xin = _fit(hspy_comp=hspy_comp)
    kept = {a: np.array(getattr(est, a), copy=True) for a in ("W_", "H_", "G_", "components_", "X_")}
    est.pixel_diagnostics(X=Xin)
    out = est.presence_maps(X=Xin, max_pass=4000)
    k, p = 3, 300
    assert est.H_ml_.shape == (k, p) and est.H_ml_.dtype == np.float64 and est.deviance_ml_.shape == (p,)
    assert est.presence_lr_.shape == est.presence_pvalue_.shape == (k, p) and est.presence_lr_.dtype == np.float64
    assert est.ml_converged_.shape == est.ml_gap_.shape == est.ml_n_pass_.shape == (k + 1, p)
    assert est.ml_converged_.dtype == bool and est.ml_n_pass_.dtype.kind == "i"
    assert out["H_ml"].shape == ((p, k) if hspy_comp else (k, p)) and out["lr"] is est.presence_lr_
    # the ML over a bigger feasible set cannot fit worse than the fit (EM from H_ never raises the deviance, converged or not)
    print(f"deviance_ - deviance_ml_ in [{np.min(est.deviance_ - est.deviance_ml_):.3g}, {np.max(est.deviance_ - est.deviance_ml_):.3g}], "
          f"{est.ml_converged_.mean():.3f} converged, passes <= {est.ml_n_pass_.max()}")
    assert (est.deviance_ml_ <= est.deviance_ + 1e-3).all()
    assert (est.presence_lr_ >= 0).all() and (est.presence_pvalue_[est.presence_lr_ == 0] == 1).all()
    G, W, _ = est._model_factors()
    D = W if G is None else G @ W
    want = presence.presence(Xin, D, np.asarray(est.H_, dtype=np.float64), max_pass=4000, log_shift=est.log_shift, layout="pm" if hspy_comp else "cm")
    assert np.array_equal(want["lr"], est.presence_lr_) and np.array_equal(want["H_ml"], est.H_ml_)
    h, lr, pv = ha.presence_maps(est)
    assert h.shape == lr.shape == pv.shape == (k,) + SHAPE and np.array_equal(lr.reshape(k, p), est.presence_lr_)
    for a, v in kept.items():
        assert np.array_equal(np.asarray(getattr(est, a)), v), a


def test_estimator_with_simplex_H_runs_and_maps_the_dose(presence):
    est, Xin = _fit(simplex_H=True)
    assert est.simplex_H and np.allclose(est.H_.sum(axis=0), 1.0, atol=1e-4)
    est.presence_maps(X=Xin, max_pass=4000)
    N = Xin.sum(axis=0).astype(np.float64)
    G, W, _ = est._model_factors()
    s = (W if G is None else G @ W).sum(axis=0)
    live = N > 0
    np.testing.assert_allclose((s @ est.H_ml_)[live], N[live], rtol=1e-12)   # the pixel's scale is free: the ML carries its counts
    assert np.isfinite(est.H_ml_).all() and est.presence_lr_.shape == (3, 300)
