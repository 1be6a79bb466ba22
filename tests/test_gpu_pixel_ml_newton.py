"""The Newton rule of the pixel ML on the device (csrc/mu_pixel_ml_newton.hip, ``method="newton"`` of espm_amd/presence.py).  As in
test_gpu_pixel_ml.py the correctness checks are SOLVER-AGNOSTIC: the certificate is recomputed in numpy from the returned h, and the
optimum it is held against comes from the EM reference's long run.  The path is compared with the rule's numpy restatement
(tests/pixel_ml_newton_reference.py) only in its length: an accept / reject tie may fall the other way under the kernel's fma order,
after which the paths differ and the certified ends do not.  What the kernel promises bit for bit - both layouts, every dtype, every
split into calls, padded rows, slabs - is compared with ``np.array_equal``.  test_pixel_ml_newton_cpu.py holds what all of this rests
on: the reference alone converges everywhere within half of MAX_PASS = 128, and EM does not."""
import ctypes as C
import functools

import numpy as np
import pytest

import pixel_ml_newton_reference as nr
import pixel_ml_reference as pr

pytestmark = pytest.mark.gpu

TOL = 1e-3
KEYS = ("H", "deviance", "gap", "n_pass", "converged")
BITS = ("img96_k5", "tall", "low8")


@pytest.fixture(scope="module")
def presence():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import presence
    return presence


def _unmix(X, D, H0, layout="cm", **kw):
    from espm_amd import presence
    kw.setdefault("max_pass", nr.MAX_PASS)
    kw.setdefault("method", "newton")
    return presence.ml_unmix(X, D, H0, tol=kw.pop("tol", TOL), layout=layout, **kw)


@functools.lru_cache(maxsize=None)
def _solved(name, layout="cm"):
    """The device's fit of a named case from the reference's start (shared: read-only)."""
    X, D = nr.case(name)
    return _unmix(X if layout == "cm" else np.ascontiguousarray(X.T), D, nr.start_from(X, D), layout)


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys) and a["unmodelled"] == b["unmodelled"]


def _certified(X, D, got, components=None):
    """The checks every returned point passes, whatever the path: the certificate and the deviance recomputed in numpy from H."""
    M = pr.mask_of(D.shape[1], components)
    ev = pr.evaluate(X, D, got["H"], M)
    N, live = ev["N"], ev["N"] > 0
    assert got["converged"].all() and got["nonfinite"] == 0
    assert (ev["gap"][live] <= TOL * (1 + 1e-9)).all() and (got["gap"] <= TOL).all()
    assert (np.abs(got["deviance"] - ev["deviance"])[live] <= 1e-9 * np.abs(ev["deviance"][live])).all()
    assert not got["H"][~M].any() and (got["H"] >= 0).all() and not got["H"][:, ~live].any()
    np.testing.assert_allclose((D.sum(axis=0) @ got["H"])[live], N[live], rtol=1e-14)   # h as scaled in step 1
    return ev


# ---- solver-agnostic correctness ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("name", nr.CASES)
def test_certificate_recomputed_in_numpy(presence, name, layout):
    X, D = nr.case(name)
    got, ref, opt = _solved(name, layout), nr.solved(name), nr.optimum(name)
    assert got["H"].shape == (D.shape[1], X.shape[1]) and got["n_pass"].dtype.kind == "i" and got["converged"].dtype == bool
    n = got["n_pass"]
    print(f"{name} {layout}: passes max {n.max()} (reference {ref['n_pass'].max()}), sum {n.sum()} (reference {ref['n_pass'].sum()}), "
          f"{(n != ref['n_pass']).sum()} pixels differ; dev - dev_opt <= {np.max(got['deviance'] - opt['deviance']):.3g}")
    ev = _certified(X, D, got)
    assert got["unmodelled"] == 0
    assert (got["deviance"] <= opt["deviance"] + TOL).all()
    # the path's length: the margin covers accept / reject ties under the kernel's fma order (the reference under a second order: none)
    assert n.sum() <= 1.25 * ref["n_pass"].sum() and n.max() <= nr.MAX_PASS // 2
    assert (n[ev["N"] == 0] == 0).all()


def test_newton_converges_the_planted_image_where_em_with_the_same_cap_does_not(presence):
    X, D = nr.case("planted")
    H0 = nr.start_from(X, D)
    assert _solved("planted")["converged"].all()
    em = _unmix(X, D, H0, method="em")
    print(f"EM: {em['converged'].sum()} of {em['converged'].size} pixels converged within {nr.MAX_PASS} passes")
    assert not em["converged"].all() and (em["n_pass"][~em["converged"]] == nr.MAX_PASS).all()
    explicit = presence.ml_unmix(X, D, H0, max_pass=nr.MAX_PASS)   # the default stays EM
    assert _same(explicit, em)


# ---- what is promised bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BITS)
def test_both_layouts_and_every_dtype_give_the_same_bits(presence, name):
    X, D = nr.case(name)
    H0, want = nr.start_from(X, D), _solved(name)
    assert _same(_solved(name, "pm"), want)
    for dtype in (np.uint16, np.float32, np.float64):
        assert _same(_unmix(X.astype(dtype), D, H0), want), dtype
        assert _same(_unmix(np.ascontiguousarray(X.T).astype(dtype), D, H0, layout="pm"), want), dtype


@pytest.mark.parametrize("name", BITS)
def test_the_split_into_calls_does_not_matter(presence, name):
    X, D = nr.case(name)
    H0, want = nr.start_from(X, D), _solved(name)
    assert want["n_pass"].max() >= 2   # (more than one chunk of 1)
    for chunk in (1, 7, 64):
        assert _same(_unmix(X, D, H0, chunk=chunk), want), chunk


@pytest.mark.parametrize("name", BITS)
def test_padded_rows_and_two_slabs(presence, name):
    import torch
    X, D = nr.case(name)
    H0, want = nr.start_from(X, D), _solved(name)
    p = X.shape[1]
    for layout, Xl in (("cm", X), ("pm", np.ascontiguousarray(X.T))):
        wide = torch.zeros((Xl.shape[0], Xl.shape[1] + 13), dtype=torch.uint8, device="cuda")
        wide[:, :Xl.shape[1]] = torch.from_numpy(Xl).cuda()
        view = wide[:, :Xl.shape[1]]
        assert view.stride(0) == Xl.shape[1] + 13
        assert _same(_unmix(view, D, H0, layout=layout), want), layout
    # two slabs against one call: an odd cut, the second slab a view into the whole image on the device (ld = p)
    cut = p // 3 | 1
    whole = torch.from_numpy(np.array(X)).cuda()
    first, second = _unmix(np.ascontiguousarray(X[:, :cut]), D, H0[:, :cut]), _unmix(whole[:, cut:], D, H0[:, cut:])
    assert all(np.array_equal(np.concatenate([first[k], second[k]], axis=-1), want[k]) for k in KEYS)
    pm = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    assert all(np.array_equal(_unmix(pm[cut:], D, H0[:, cut:], layout="pm")[k], want[k][..., cut:]) for k in KEYS)


# ---- the state rules, through the entry point itself --------------------------------------------------------------------------------------
class _Raw:
    """The entry point on device tensors of the caller: the state is in plain sight."""

    def __init__(self, name):
        import torch

        from espm_amd import _lib
        X, D = nr.case(name)
        self.n, self.p, self.k = X.shape[0], X.shape[1], D.shape[1]
        self.s = np.ascontiguousarray(D.sum(axis=0))
        self.X, self.D = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(D)).cuda()
        self.H = torch.from_numpy(np.ascontiguousarray(nr.start_from(X, D))).cuda()
        self.dev, self.gap = (torch.full((self.p,), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
        self.passes = torch.zeros(self.p, dtype=torch.int32, device="cuda")
        self.done = torch.zeros(self.p, dtype=torch.uint8, device="cuda")
        self.counters = torch.zeros(3, dtype=torch.int64, device="cuda")
        self.extra = torch.full((self.k + _lib.PMLN_STATE_EXTRA, self.p), -3.0, dtype=torch.float64, device="cuda")   # (never read before written)

    def call(self, n_pass, tol=TOL):
        from espm_amd import _lib
        from espm_amd.engine import _ptr, _stream
        rc = _lib.lib.espm_pixel_ml_newton(_ptr(self.X), _lib.DIAG_X_U8, _lib.LAYOUT_CM, self.p, self.n, self.p, _ptr(self.D),
                                           self.s.ctypes.data_as(C.c_void_p), self.k, (1 << self.k) - 1, 1e-14, tol, n_pass, _ptr(self.H),
                                           _ptr(self.dev), _ptr(self.gap), _ptr(self.passes), _ptr(self.done), _ptr(self.counters),
                                           _ptr(self.extra), self.extra.numel() * 8, _stream())
        _lib.check(rc)
        return self

    def state(self):
        return tuple(t.cpu().numpy().copy() for t in (self.H, self.dev, self.gap, self.passes, self.done, self.counters))


def test_resumable_and_a_done_pixel_is_never_touched(presence):
    one = _Raw("planted").call(9).state()
    two = _Raw("planted").call(4)
    mid = two.state()
    then = two.call(5).state()
    assert all(np.array_equal(a, b) for a, b in zip(one, then))   # 4 + 5 passes: the bits of 9, counters included
    done_mid = mid[4] == 1
    assert 0 < done_mid.sum() < done_mid.size and 0 < (then[4] == 1).sum() < done_mid.size   # (some done after 4, not all after 9)
    assert then[5][0] == (then[4] == 0).sum() and mid[5][0] == (mid[4] == 0).sum()           # the one integer the host loop reads
    for a, b in zip(mid[:5], then[:5]):
        assert np.array_equal(a[..., done_mid], b[..., done_mid])
    left = then[4] == 0
    assert (then[3][left] == 9).all() and (then[2][left] > TOL).all() and (then[2][then[4] == 1] <= TOL).all()
    # a pixel still running reports its last ACCEPTED point: a deviance that only ever fell from call to call
    assert (then[1][left] <= mid[1][left]).all() and np.isfinite(then[0]).all()
    # all done: a further call writes nothing at all
    full = _Raw("img96_k2").call(nr.MAX_PASS)
    before = full.state()
    assert before[5][0] == 0 and (before[4] == 1).all()
    full.H += 1.0   # (were a done pixel rewritten, its h would come back scaled)
    after = full.call(50).state()
    assert np.array_equal(after[0], before[0] + 1.0) and all(np.array_equal(a, b) for a, b in zip(before[1:], after[1:]))


def test_a_cap_too_small_leaves_the_next_start_and_the_accepted_point(presence):
    X, D = nr.case("low8")
    H0 = nr.start_from(X, D)
    out = _unmix(X, D, H0, max_pass=5)
    left = ~out["converged"]
    assert 0 < left.sum() < left.size
    assert (out["gap"][left] > TOL).all() and (out["n_pass"][left] == 5).all() and (out["n_pass"][~left] < 5).all()
    assert np.isfinite(out["H"]).all() and (out["H"][:, left] > 0).all() and np.isfinite(out["deviance"]).all()
    assert _same(_unmix(X, D, H0, max_pass=5, chunk=2), out)
    # the h a pixel holds at the cap is the start of its next pass: carried on from there, every pixel ends certified
    more = _unmix(X, D, out["H"])
    _certified(X, D, more)


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------------
def test_a_pixel_without_counts_and_one_component(presence):
    X, D = nr.case("planted")
    got = _solved("planted")
    assert not X[:, 5].any()
    assert not got["H"][:, 5].any() and got["deviance"][5] == 0 and got["gap"][5] == 0 and got["n_pass"][5] == 0 and got["converged"][5]
    one = _solved("img96_k1")   # k = 1: the scale of step 1 is the answer, no pass is counted
    _certified(*nr.case("img96_k1"), one)
    X1, D1 = nr.case("img96_k1")
    assert not one["n_pass"].any() and _same(one, _unmix(X1, D1, nr.start_from(X1, D1), method="em"))   # the stop comes before any step


def test_a_component_subset_and_starts_that_are_not_positive(presence):
    X, D = nr.case("img96_k8")
    H0, comp = nr.start_from(X, D), [1, 4, 6]
    sub, ref = _unmix(X, D, H0, components=comp), nr.ml_unmix(X, D, H0, comp, TOL)
    _certified(X, D, sub, comp)
    assert (sub["deviance"] <= ref["deviance"] + TOL).all()   # certified: within tol of the minimum, which no point is below
    assert sub["n_pass"].sum() <= 1.25 * ref["n_pass"].sum() and sub["n_pass"].max() <= nr.MAX_PASS // 2
    assert _same(_unmix(np.ascontiguousarray(X.T), D, H0, layout="pm", components=comp), sub)
    # entries of the start that are not > 0 (zero, negative) become N / (|M| s_j) * 1e-3: the same bits as that start given outright
    N, s = X.sum(axis=0).astype(np.float64), D.sum(axis=0)
    holes = H0.copy()
    holes[1, ::3], holes[6, 1::4], holes[0] = 0.0, -1.0, 5.0
    filled = holes.copy()
    for j in (1, 6):
        bad = ~(holes[j] > 0)
        filled[j, bad] = (N / (3.0 * s[j]) * 1e-3)[bad]
    got = _unmix(X, D, holes, components=comp)
    _certified(X, D, got, comp)
    assert _same(got, _unmix(X, D, filled, components=comp))
    # no start at all: N / sum_M s
    _certified(X, D, _unmix(X, D, None))


def test_refusals(presence):
    X, D = nr.case("planted")
    Dz = np.array(D)
    Dz[:, 1] = 0.0
    with pytest.raises(ValueError, match="component 1"):
        _unmix(X, Dz, None)
    raw = _Raw("planted")
    raw.s[1] = 0.0
    with pytest.raises(ValueError, match="component 1"):
        raw.call(1)
    out = _unmix(X, Dz, nr.start_from(X, Dz), components=[0, 2, 3])   # outside the set an all-zero spectrum is nobody's business
    _certified(X, Dz, out, [0, 2, 3])
    with pytest.raises(NotImplementedError, match="9 components"):
        _unmix(np.zeros((6, 10), np.float32), np.ones((6, 9)), None)
    with pytest.raises(ValueError, match="method"):
        _unmix(X, D, None, method="bogus")


# ---- presence -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planted", "img96_k3"])
def test_presence_against_the_em_reference(presence, name):
    """Both deviances of a pair lie within tol of their minima under either method, and max(., 0) is 1-Lipschitz: the statistic of the
    Newton rule is within 2 tol of the EM reference's."""
    X, D = nr.case(name)
    k, p = D.shape[1], X.shape[1]
    out = presence.presence(X, D, tol=TOL, max_pass=nr.MAX_PASS, method="newton")
    ref = pr.presence(X, D, None, TOL, pr.MAX_PASS)
    assert ref["converged"].all()
    print(f"{name}: |lr - lr_EM| <= {np.max(np.abs(out['lr'] - ref['lr'])):.3g}; passes per fit <= {out['n_pass'].max(axis=1)}")
    assert out["lr"].shape == out["pvalue"].shape == (k, p) and out["converged"].shape == out["gap"].shape == out["n_pass"].shape == (k + 1, p)
    assert out["converged"].all() and (out["gap"] <= TOL).all() and out["nonfinite"] == 0
    assert (np.abs(out["lr"] - ref["lr"]) <= 2 * TOL).all()
    assert np.array_equal(out["pvalue"], pr.pvalue(out["lr"]))
    full = _unmix(X, D, None)
    assert np.array_equal(out["n_pass"][0], full["n_pass"]) and np.array_equal(out["H_ml"], full["H"])   # row 0 is the full fit
    assert np.array_equal(out["deviance_ml"], full["deviance"]) and out["n_pass"].max() <= nr.MAX_PASS // 2


# ---- the estimator and the adapter --------------------------------------------------------------------------------------------------------
SHAPE = (15, 20)
ATTRS = ("H_ml_", "deviance_ml_", "presence_lr_", "presence_pvalue_", "ml_converged_", "ml_gap_", "ml_n_pass_")


def _fit(hspy_comp=False):
    from espm_amd.estimators import SmoothNMF
    X = nr.case("planted")[0]
    est = SmoothNMF(n_components=3, max_iter=200, tol=0.0, verbose=0, random_state=0, shape_2d=SHAPE, simplex_H=False, simplex_W=True, hspy_comp=hspy_comp)
    Xin = np.ascontiguousarray(X.T) if hspy_comp else X
    est.fit(Xin.astype(np.float32))
    return est, Xin


@pytest.mark.parametrize("hspy_comp", [False, True], ids=["cm", "hspy"])
def test_estimator_and_adapter(presence, hspy_comp):
    from espm_amd import hyperspy_adapter as ha
    est, Xin = _fit(hspy_comp)
    est.pixel_diagnostics(X=Xin)
    out = est.presence_maps(X=Xin, max_pass=nr.MAX_PASS, method="newton")
    k, p = 3, 300
    assert all(hasattr(est, a) for a in ATTRS) and est.ml_method_ == "newton"
    assert est.H_ml_.shape == (k, p) and est.deviance_ml_.shape == (p,) and est.presence_lr_.shape == est.presence_pvalue_.shape == (k, p)
    assert est.ml_converged_.shape == est.ml_gap_.shape == est.ml_n_pass_.shape == (k + 1, p)
    assert est.ml_converged_.all() and est.ml_n_pass_.max() <= nr.MAX_PASS // 2
    assert out["H_ml"].shape == ((p, k) if hspy_comp else (k, p)) and out["lr"] is est.presence_lr_
    print(f"deviance_ - deviance_ml_ in [{np.min(est.deviance_ - est.deviance_ml_):.3g}, {np.max(est.deviance_ - est.deviance_ml_):.3g}], "
          f"passes <= {est.ml_n_pass_.max()}")
    assert (est.deviance_ml_ <= est.deviance_ + TOL).all()   # the ML over a bigger feasible set, certified to tol
    G, W, _ = est._model_factors()
    D = W if G is None else G @ W
    want = presence.presence(Xin, D, np.asarray(est.H_, dtype=np.float64), max_pass=nr.MAX_PASS, log_shift=est.log_shift,
                             layout="pm" if hspy_comp else "cm", method="newton")
    assert np.array_equal(want["lr"], est.presence_lr_) and np.array_equal(want["H_ml"], est.H_ml_)
    newton_lr = est.presence_lr_
    h, lr, pv = ha.presence_maps(est)
    assert h.shape == lr.shape == pv.shape == (k,) + SHAPE and np.array_equal(lr.reshape(k, p), newton_lr)
    # the default is EM, and says so; the two statistics agree within the two certificates
    est.presence_maps(X=Xin, max_pass=4000)
    ok = est.ml_converged_.all(axis=0)   # (EM may leave pixels at this cap)
    assert est.ml_method_ == "em" and ok.any()
    assert (np.abs(est.presence_lr_ - newton_lr)[:, ok] <= 2 * TOL).all()
    # the adapter passes the method through (on the fit's own image)
    assert ha.presence_maps(est, method="newton")[1].shape == (k,) + SHAPE and est.ml_method_ == "newton"
