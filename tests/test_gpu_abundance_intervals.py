"""The pinned pixel ML on the device (csrc/mu_pixel_ml_pinned.hip) and the profile-likelihood intervals built on it
(``presence.ml_unmix_pinned``, ``presence.intervals``, ``est.abundance_intervals``, ``hyperspy_adapter.abundance_interval_maps``).
The correctness checks are SOLVER-AGNOSTIC: deviance, certificate and slope are recomputed in numpy from the returned h, the optima
they are held against come from the numpy restatement's long runs (tests/pixel_ml_pinned_reference.py, tol = 1e-10), and the path
is compared with the restatement only in its length.  What the kernel promises bit for bit - both layouts, every dtype, every split
into calls, padded rows, slabs - is compared with ``np.array_equal``.  test_pixel_ml_pinned_cpu.py holds what all of this rests on:
the reference alone converges every pinned fit within half of MAX_PASS = 128 and every end within half of MAX_EVAL = 64."""
import ctypes as C
import functools

import numpy as np
import pytest

import pixel_ml_pinned_reference as pn

pytestmark = pytest.mark.gpu

TOL = 1e-3
LR_TOL = 1e-2
KEYS = ("H", "deviance", "gap", "slope", "n_pass", "converged")
BITS = ("img96_k5", "tall", "low8")


@pytest.fixture(scope="module")
def presence():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import presence
    return presence


def _pin(name):
    return pn.case(name)[1].shape[1] - 1


def _unmix(X, D, pin, t, H0, layout="cm", **kw):
    from espm_amd import presence
    kw.setdefault("max_pass", pn.MAX_PASS)
    return presence.ml_unmix_pinned(X, D, pin, t, H0, tol=kw.pop("tol", TOL), layout=layout, **kw)


@functools.lru_cache(maxsize=None)
def _fitted(name, label, layout="cm"):
    """The device's pinned fit of the last component of a named case at one of the reference's values, from the reference's full
    solution (shared: read-only)."""
    X, D = pn.case(name)
    return _unmix(X if layout == "cm" else np.ascontiguousarray(X.T), D, _pin(name), pn.pins(name)[label], pn.solved(name)["H_ml"], layout)


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys) and a["unmodelled"] == b["unmodelled"]


def _certified(X, D, got, pin, t, components=None):
    """The checks every returned point passes, whatever the path: deviance, certificate and slope recomputed in numpy from H.  The
    slack of the two recomputed sums: n <= 300 terms of relative rounding 1.1e-16 on magnitudes N (the certificate) and
    2 (s_pin + q_pin) (the slope) - 1e-9 of those is far above it and far below tol."""
    k = D.shape[1]
    ev = pn.evaluate(X, D, got["H"], pin, components)
    M = pn.mask_of(k, [j for j in range(k) if j != pin] if components is None else components)
    s = D.sum(axis=0)
    assert got["converged"].all() and got["nonfinite"] == 0
    assert (got["gap"] <= TOL).all() and (ev["gap"] <= TOL + 1e-9 * np.maximum(1.0, ev["N"])).all()
    assert (np.abs(got["gap"] - ev["gap"]) <= 1e-9 * np.maximum(1.0, ev["N"])).all()
    assert (np.abs(got["deviance"] - ev["deviance"]) <= 1e-9 * np.abs(ev["deviance"])).all()
    assert (np.abs(got["slope"] - ev["slope"]) <= 1e-9 * (1.0 + 4.0 * s[pin] + np.abs(ev["slope"]))).all()
    assert np.array_equal(got["H"][pin], np.broadcast_to(t, got["H"][pin].shape))   # bit for bit
    rest = ~M
    rest[pin] = False
    assert not got["H"][rest].any() and (got["H"] >= 0).all() and np.isfinite(got["H"]).all()
    assert not got["H"][M][:, ev["N"] == 0].any()
    return ev


# ---- solver-agnostic correctness of a pinned fit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", pn.LABELS)
@pytest.mark.parametrize("name", pn.CASES)
def test_pinned_fit_recomputed_in_numpy(presence, name, label):
    X, D = pn.case(name)
    got, ref, opt = _fitted(name, label), pn.pinned(name, label), pn.pinned(name, label, 1e-10)
    assert got["H"].shape == (D.shape[1], X.shape[1]) and got["slope"].shape == (X.shape[1],) and got["converged"].dtype == bool
    n = got["n_pass"]
    print(f"{name} {label}: passes max {n.max()} (reference {ref['n_pass'].max()}), sum {n.sum()} (reference {ref['n_pass'].sum()}); "
          f"dev - dev_opt <= {np.max(got['deviance'] - opt['deviance']):.3g}")
    _certified(X, D, got, _pin(name), pn.pins(name)[label])
    assert opt["converged"].all() and (got["deviance"] <= opt["deviance"] + TOL).all()
    assert n.sum() <= 1.25 * ref["n_pass"].sum() and n.max() <= pn.MAX_PASS // 2


def test_img96_k5_in_the_pixel_major_layout(presence):
    for label in pn.LABELS:
        assert _same(_fitted("img96_k5", label, "pm"), _fitted("img96_k5", label))


def test_a_component_subset_a_scalar_value_and_no_start(presence):
    X, D = pn.case("low8")
    comp, pin = [1, 4, 6], 3
    got = _unmix(X, D, pin, 0.25, None, components=comp)
    _certified(X, D, got, pin, 0.25, comp)
    opt = pn.ml_unmix_pinned(X, D, pin, 0.25, None, comp, 1e-10, 20000)
    assert opt["converged"].all() and (got["deviance"] <= opt["deviance"] + TOL).all()
    assert _same(_unmix(np.ascontiguousarray(X.T), D, pin, np.full(X.shape[1], 0.25), None, "pm", components=comp), got)
    # the empty set by the caller's choice: nothing is fitted, the pixel is done in its first pass
    none = _unmix(X, D, pin, 0.25, None, components=[])
    ev = _certified(X, D, none, pin, 0.25, [])
    assert not none["n_pass"].any() and not none["gap"].any() and not np.delete(none["H"], pin, axis=0).any()
    assert np.array_equal(ev["gap"], np.zeros_like(ev["gap"]))


# ---- what is promised bit for bit ---------------------------------------------------------------------------------------------------------
def _args(name):
    X, D = pn.case(name)
    return X, D, _pin(name), pn.pins(name)["twice"], pn.solved(name)["H_ml"], _fitted(name, "twice")


@pytest.mark.parametrize("name", BITS)
def test_both_layouts_and_every_dtype_give_the_same_bits(presence, name):
    X, D, pin, t, H0, want = _args(name)
    assert _same(_fitted(name, "twice", "pm"), want)
    for dtype in (np.uint16, np.float32, np.float64):
        assert _same(_unmix(X.astype(dtype), D, pin, t, H0), want), dtype
        assert _same(_unmix(np.ascontiguousarray(X.T).astype(dtype), D, pin, t, H0, "pm"), want), dtype


@pytest.mark.parametrize("name", BITS)
def test_the_split_into_calls_does_not_matter(presence, name):
    X, D, pin, t, H0, want = _args(name)
    assert want["n_pass"].max() >= 2   # (more than one chunk of 1)
    for chunk in (1, 7, 64):
        assert _same(_unmix(X, D, pin, t, H0, chunk=chunk), want), chunk


@pytest.mark.parametrize("name", BITS)
def test_padded_rows_and_two_slabs(presence, name):
    import torch
    X, D, pin, t, H0, want = _args(name)
    p = X.shape[1]
    for layout, Xl in (("cm", X), ("pm", np.ascontiguousarray(X.T))):
        wide = torch.zeros((Xl.shape[0], Xl.shape[1] + 13), dtype=torch.uint8, device="cuda")
        wide[:, :Xl.shape[1]] = torch.from_numpy(Xl).cuda()
        view = wide[:, :Xl.shape[1]]
        assert view.stride(0) == Xl.shape[1] + 13
        assert _same(_unmix(view, D, pin, t, H0, layout), want), layout
    # two slabs against one call: an odd cut, t sliced with the pixels, the second slab a view into the whole image on the device
    cut = p // 3 | 1
    whole = torch.from_numpy(np.array(X)).cuda()
    first = _unmix(np.ascontiguousarray(X[:, :cut]), D, pin, t[:cut], H0[:, :cut])
    second = _unmix(whole[:, cut:], D, pin, t[cut:], H0[:, cut:])
    assert all(np.array_equal(np.concatenate([first[k], second[k]], axis=-1), want[k]) for k in KEYS)
    pm = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    assert all(np.array_equal(_unmix(pm[cut:], D, pin, t[cut:], H0[:, cut:], "pm")[k], want[k][..., cut:]) for k in KEYS)


# ---- the state rules, through the entry point itself --------------------------------------------------------------------------------------
class _Raw:
    """The entry point on device tensors of the caller: the state is in plain sight, and every output starts as garbage."""

    def __init__(self, name, label="twice"):
        import torch

        from espm_amd import _lib
        X, D = pn.case(name)
        self.n, self.p, self.k = X.shape[0], X.shape[1], D.shape[1]
        self.pin = self.k - 1
        self.s = np.ascontiguousarray(D.sum(axis=0))
        self.X, self.D = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(D)).cuda()
        self.H = torch.from_numpy(np.ascontiguousarray(pn.start_from(X, D))).cuda()
        self.t = torch.from_numpy(np.ascontiguousarray(pn.pins(name)[label])).cuda()
        self.dev, self.gap, self.slope = (torch.full((self.p,), -7.0, dtype=torch.float64, device="cuda") for _ in range(3))
        self.passes = torch.zeros(self.p, dtype=torch.int32, device="cuda")
        self.done = torch.zeros(self.p, dtype=torch.uint8, device="cuda")
        self.counters = torch.zeros(3, dtype=torch.int64, device="cuda")
        self.extra = torch.full((self.k + _lib.PMLN_STATE_EXTRA, self.p), float("nan"), dtype=torch.float64, device="cuda")   # (never read before written)

    def call(self, n_pass, tol=TOL):
        from espm_amd import _lib
        from espm_amd.engine import _ptr, _stream
        mask = ((1 << self.k) - 1) & ~(1 << self.pin)
        rc = _lib.lib.espm_pixel_ml_pinned(_ptr(self.X), _lib.DIAG_X_U8, _lib.LAYOUT_CM, self.p, self.n, self.p, _ptr(self.D),
                                           self.s.ctypes.data_as(C.c_void_p), self.k, mask, self.pin, _ptr(self.t), 1e-14, tol, n_pass,
                                           _ptr(self.H), _ptr(self.dev), _ptr(self.gap), _ptr(self.slope), _ptr(self.passes), _ptr(self.done),
                                           _ptr(self.counters), _ptr(self.extra), self.extra.numel() * 8, _stream())
        _lib.check(rc)
        return self

    def state(self):
        return tuple(t.cpu().numpy().copy() for t in (self.H, self.dev, self.gap, self.slope, self.passes, self.done, self.counters, self.extra))


def test_resumable_garbage_state_and_a_done_pixel_is_never_touched(presence):
    one = _Raw("planted").call(7).state()
    two = _Raw("planted").call(3)
    mid = two.state()
    then = two.call(4).state()
    # 3 + 4 passes: the bits of 7, counters included; the state (NaN before the first call) compares equal where it was written
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(one, then))
    assert np.isfinite(then[0]).all() and np.isfinite(then[1]).all() and np.isfinite(then[2]).all() and np.isfinite(then[3]).all()
    done_mid = mid[5] == 1
    assert 0 < done_mid.sum() < done_mid.size and 0 < (then[5] == 1).sum() < done_mid.size   # (some done after 3, not all after 7)
    assert then[6][0] == (then[5] == 0).sum() and mid[6][0] == (mid[5] == 0).sum()           # the one integer the host loop reads
    for a, b in zip(mid[:6], then[:6]):
        assert np.array_equal(a[..., done_mid], b[..., done_mid])
    left = then[5] == 0
    assert (then[4][left] == 7).all() and (then[2][left] > TOL).all() and (then[2][then[5] == 1] <= TOL).all()
    assert (then[1][left] <= mid[1][left]).all()   # a pixel still running reports its last ACCEPTED point
    # pixels the caller retired before the first call: everything of theirs keeps its bits, garbage included
    raw = _Raw("planted")
    raw.done[::3] = 1
    before = raw.state()
    after = raw.call(pn.MAX_PASS).state()
    gone = before[5] == 1
    for a, b in zip(before[:6] + before[7:], after[:6] + after[7:]):
        assert np.array_equal(a[..., gone], b[..., gone], equal_nan=True)
    assert (after[5][~gone] == 1).all() and after[6][0] == 0
    full = _Raw("planted").call(pn.MAX_PASS).state()
    for a, b in zip(full[:5], after[:5]):   # ... and the others do not notice
        assert np.array_equal(a[..., ~gone], b[..., ~gone])
    # all done: a further call writes nothing at all
    raw.H += 1.0
    again = raw.call(50).state()
    assert np.array_equal(again[0], after[0] + 1.0) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(after[1:], again[1:]))


def test_a_value_that_is_negative_or_not_finite_stops_the_pixel(presence):
    raw = _Raw("planted")
    raw.t[3], raw.t[7], raw.t[11] = -1.0, float("nan"), float("inf")
    H0 = raw.H.cpu().numpy().copy()
    out = raw.call(pn.MAX_PASS).state()
    bad = np.zeros(raw.p, dtype=bool)
    bad[[3, 7, 11]] = True
    assert (out[5][bad] == 2).all() and (out[5][~bad] == 1).all() and out[6][2] == 3 and out[6][0] == 0
    assert np.array_equal(out[0][:, bad], H0[:, bad]) and not out[4][bad].any()
    assert not out[1][bad].any() and not out[2][bad].any() and not out[3][bad].any()


# ---- intervals ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _intervals(name, layout="cm"):
    from espm_amd import presence
    X, D = pn.case(name)
    return presence.intervals(X if layout == "cm" else np.ascontiguousarray(X.T), D, max_pass=pn.MAX_PASS, layout=layout)


@pytest.mark.parametrize("name", pn.CASES)
def test_interval_ends_against_the_long_runs(presence, name):
    """|g*(t) - dev* - q| <= lr_tol + tol + 1e-9 dev* at every end the root finder placed: each reported deviance lies within its
    gap <= tol above its minimum, and the stop is lr_tol on the reported values.  An end at exactly 0 is the boundary: there the
    profile has not reached the level, g*(0) - dev* - q <= the same bound."""
    X, D = pn.case(name)
    k, p = D.shape[1], X.shape[1]
    got, ref, q = _intervals(name), pn.solved(name), pn.threshold(0.95)
    assert got["lower"].shape == got["upper"].shape == (k, p) and got["converged"].shape == got["n_eval"].shape == got["n_pass"].shape == (k, 2, p)
    assert got["converged"].dtype == bool and got["level"] == 0.95 and abs(got["threshold"] - q) <= 1e-12 and got["nonfinite"] == 0
    print(f"{name}: evaluations per end <= {got['n_eval'].max()} (reference {ref['n_eval'].max()}), passes {got['n_pass'].sum()} "
          f"(reference {ref['n_pass'].sum()}); lower == 0 in {np.mean(got['lower'] == 0):.3f} of the entries")
    assert got["converged"].all() and np.isfinite(got["lower"]).all() and np.isfinite(got["upper"]).all()
    assert got["n_eval"].max() <= 32 and got["n_pass"].sum() <= 1.25 * ref["n_pass"].sum()
    assert (got["lower"] <= got["H_ml"]).all() and (got["H_ml"] <= got["upper"]).all() and (got["lower"] >= 0).all()
    dev_opt = pn.full_optimum(name)["deviance"]
    bound = LR_TOL + TOL + 1e-9 * dev_opt
    worst = 0.0
    for j in range(k):
        rest = [i for i in range(k) if i != j]
        for side, end in ((0, got["lower"][j]), (1, got["upper"][j])):
            opt = pn.ml_unmix_pinned(X, D, j, end, got["H_ml"], rest, 1e-10, 20000)
            assert opt["converged"].all()
            phi = opt["deviance"] - dev_opt - q
            at_zero = (end == 0) if side == 0 else np.zeros(p, dtype=bool)
            worst = max(worst, float(np.abs(phi[~at_zero]).max(initial=0.0)))
            assert (np.abs(phi[~at_zero]) <= bound[~at_zero]).all(), (j, side)
            assert (phi[at_zero] <= bound[at_zero]).all(), (j, side)
    print(f"{name}: |g*(t) - dev* - q| <= {worst:.3g}")


def test_img96_k5_intervals_in_the_pixel_major_layout(presence):
    a, b = _intervals("img96_k5", "pm"), _intervals("img96_k5")
    assert all(np.array_equal(a[key], b[key]) for key in ("H_ml", "deviance_ml", "lower", "upper", "converged", "n_eval", "n_pass"))


@pytest.mark.parametrize("name", ["planted", "low8", "collinear", "img96_k1"])
def test_lower_end_is_zero_exactly_where_the_presence_test_does_not_reject(presence, name):
    X, D = pn.case(name)
    got, q = _intervals(name), pn.threshold(0.95)
    lr = presence.presence(X, D, tol=TOL, max_pass=pn.MAX_PASS, method="newton")["lr"]
    clear = np.abs(lr - q) > 2 * TOL
    print(f"{name}: lr <= q in {np.mean(lr <= q):.3f} of the entries, {np.sum(~clear)} within 2 tol of q")
    assert np.array_equal((got["lower"] == 0)[clear], (lr <= q)[clear])


def test_the_empty_pixel_one_component_a_subset_and_the_level(presence):
    X, D = pn.case("planted")
    got, q = _intervals("planted"), pn.threshold(0.95)
    s = D.sum(axis=0)
    assert not X[:, 5].any() and (got["lower"][:, 5] == 0).all()
    assert (np.abs(got["upper"][:, 5] - q / (2 * s)) <= LR_TOL / (2 * s)).all()
    # k = 1 in closed form: the profile is 2 (t s - N - N ln(t s / N))
    one = _intervals("img96_k1")
    X1, D1 = pn.case("img96_k1")
    N, s1 = X1.sum(axis=0).astype(np.float64), D1.sum()
    for end in (one["lower"][0], one["upper"][0]):
        assert (np.abs(2.0 * (end * s1 - N - N * np.log(end * s1 / N)) - q) <= LR_TOL).all()
    assert not one["n_pass"].any()
    # a subset of the rows: the others stay NaN, the row itself does not notice
    sub = presence.intervals(X, D, components=[1], max_pass=pn.MAX_PASS)
    for key in ("lower", "upper"):
        assert np.isnan(np.delete(sub[key], 1, axis=0)).all() and np.array_equal(sub[key][1], got[key][1])
    assert not np.delete(sub["converged"], 1, axis=0).any() and not np.delete(sub["n_eval"], 1, axis=0).any() and sub["converged"][1].all()
    # the level: a narrower interval inside the wider one
    low = presence.intervals(X, D, level=0.68, components=[1], max_pass=pn.MAX_PASS)
    assert abs(low["threshold"] - 0.98895) <= 1e-4 and low["level"] == 0.68
    assert (low["upper"][1] <= got["upper"][1]).all() and (low["lower"][1] >= got["lower"][1]).all()
    # too few evaluations: the ends that did not finish are NaN and say so
    few = presence.intervals(X, D, components=[1], max_eval=2, max_pass=pn.MAX_PASS)
    left = ~few["converged"][1]
    assert left.any() and np.isnan(few["upper"][1][left[1]]).all() and (few["n_eval"][1] <= 2).all()
    assert np.isfinite(few["upper"][1][~left[1]]).all()


# ---- the estimator and the adapter --------------------------------------------------------------------------------------------------------
SHAPE = (15, 20)
ATTRS = ("H_lower_", "H_upper_", "H_interval_level_", "H_interval_converged_", "H_interval_n_eval_", "H_ml_", "deviance_ml_")
FITTED = ("W_", "H_", "G_")


def _fit(hspy_comp=False):
    from espm_amd.estimators import SmoothNMF
    X = pn.case("planted")[0]
    est = SmoothNMF(n_components=3, max_iter=200, tol=0.0, verbose=0, random_state=0, shape_2d=SHAPE, simplex_H=False, simplex_W=True, hspy_comp=hspy_comp)
    Xin = np.ascontiguousarray(X.T) if hspy_comp else X
    est.fit(Xin.astype(np.float32))
    return est, Xin


@pytest.mark.parametrize("hspy_comp", [False, True], ids=["cm", "hspy"])
def test_estimator_and_adapter(presence, hspy_comp):
    from espm_amd import hyperspy_adapter as ha
    est, Xin = _fit(hspy_comp)
    kept = {a: np.array(getattr(est, a)) for a in FITTED if getattr(est, a, None) is not None}
    out = est.abundance_intervals(X=Xin)
    k, p = 3, 300
    assert all(hasattr(est, a) for a in ATTRS) and est.H_interval_level_ == 0.95
    assert est.H_lower_.shape == est.H_upper_.shape == est.H_ml_.shape == (k, p) and est.deviance_ml_.shape == (p,)
    assert est.H_interval_converged_.shape == est.H_interval_n_eval_.shape == (k, 2, p) and est.H_interval_converged_.all()
    assert (est.H_lower_ <= est.H_ml_).all() and (est.H_ml_ <= est.H_upper_).all()
    shape = (p, k) if hspy_comp else (k, p)
    assert out["H_ml"].shape == out["lower"].shape == out["upper"].shape == shape
    assert np.array_equal(out["upper"].T if hspy_comp else out["upper"], est.H_upper_)
    for a, v in kept.items():
        assert np.array_equal(np.asarray(getattr(est, a)), v), a
    G, W, _ = est._model_factors()
    D = W if G is None else G @ W
    want = presence.intervals(Xin, D, np.asarray(est.H_, dtype=np.float64), log_shift=est.log_shift, layout="pm" if hspy_comp else "cm")
    assert np.array_equal(want["lower"], est.H_lower_) and np.array_equal(want["upper"], est.H_upper_)
    lo, up = ha.abundance_interval_maps(est)
    assert lo.shape == up.shape == (k,) + SHAPE and np.array_equal(up.reshape(k, p), est.H_upper_)
    assert ha.abundance_interval_maps(est, (20, 15))[0].shape == (k, 20, 15)
    # a one-sided 95 % upper limit is the upper end at level 0.90: inside the two-sided 95 % interval, for the requested row alone
    one = est.abundance_intervals(0.90, X=Xin, components=[2])
    assert est.H_interval_level_ == 0.90 and np.isnan(est.H_upper_[:2]).all()
    assert (est.H_upper_[2] <= up.reshape(k, p)[2]).all() and one["threshold"] < out["threshold"]
