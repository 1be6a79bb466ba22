"""The pixel ML on the simplex on the device (csrc/mu_pixel_ml_simplex.hip) and what is built on it: ``presence.ml_unmix(method=
"simplex")``, ``presence.ml_unmix_pinned(simplex=True)``, ``presence.presence(method="simplex")``, ``presence.intervals(simplex=True)``,
``est.presence_maps(method="simplex")``, ``est.abundance_intervals(simplex=True)`` and the adapter.  The correctness checks are
SOLVER-AGNOSTIC: deviance, certificate, slope and the sum are recomputed in numpy from the returned h, the optima they are held
against come from the numpy restatement's long runs (tests/pixel_ml_simplex_reference.py, tol = 1e-10), and the path is compared
with the restatement only in its length.  What the kernel promises bit for bit - both layouts, every dtype, every split into calls,
padded rows, slabs - is compared with ``np.array_equal``.  test_pixel_ml_simplex_cpu.py holds what all of this rests on: the
reference alone converges every fit within half of MAX_PASS = 128 and every end within half of MAX_EVAL = 64.

Wall time of this file on an MI355X: see DESIGN.md section 6."""
import ctypes as C
import functools

import numpy as np
import pytest

import pixel_ml_simplex_reference as sr

pytestmark = pytest.mark.gpu

TOL = 1e-3
LR_TOL = 1e-2
KEYS = ("H", "deviance", "gap", "n_pass", "converged")
PKEYS = KEYS + ("slope",)
BITS = ("img96_k5", "tall", "low8", "img96_k8")
FITTED = tuple(n for n in sr.CASES if n != "img96_k1")
POINTS = ("full",) + sr.LABELS


@pytest.fixture(scope="module")
def presence():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import presence
    return presence


def _pin(name):
    return sr.case(name)[1].shape[1] - 1


def _full(X, D, H0=None, layout="cm", **kw):
    from espm_amd import presence
    kw.setdefault("max_pass", sr.MAX_PASS)
    return presence.ml_unmix(X, D, H0, tol=kw.pop("tol", TOL), layout=layout, method="simplex", **kw)


def _unmix(X, D, pin, t, H0, layout="cm", **kw):
    from espm_amd import presence
    kw.setdefault("max_pass", sr.MAX_PASS)
    return presence.ml_unmix_pinned(X, D, pin, t, H0, tol=kw.pop("tol", TOL), layout=layout, simplex=True, **kw)


def _run(name, label, X=None, layout="cm", **kw):
    """The device's fit of a named case: ``full`` from the default start, or the last component pinned at one of the reference's
    values from the reference's full solution.  ``X``: the image in another dtype, layout or place."""
    X0, D = sr.case(name)
    X = X0 if X is None else X
    if label == "full":
        return _full(X, D, None, layout, **kw)
    return _unmix(X, D, _pin(name), sr.pins(name)[label], sr.solved(name)["H"], layout, **kw)


@functools.lru_cache(maxsize=None)
def _fitted(name, label, layout="cm"):
    """(shared: read-only)"""
    X = sr.case(name)[0]
    return _run(name, label, X if layout == "cm" else np.ascontiguousarray(X.T), layout)


def _reference(name, label, tol=1e-3):
    return sr.solved(name, tol) if label == "full" else sr.pinned(name, label, tol)


def _same(a, b):
    keys = PKEYS if "slope" in a else KEYS
    return all(np.array_equal(a[k], b[k]) for k in keys) and a["unmodelled"] == b["unmodelled"] and a["nonfinite"] == b["nonfinite"]


def _certified(X, D, got, pin=None, t=None, components=None):
    """The checks every returned point passes, whatever the path: deviance, certificate, slope and the sum recomputed in numpy from H.
    The slack of the recomputed sums: n <= 300 terms of relative rounding 1.1e-16 on the magnitudes s_j + q_j (``scale``: gap and slope
    are combinations of a few g_j = s_j - q_j with weights that add up to at most 1) - 1e-9 of those is far above it and far below
    tol."""
    k = D.shape[1]
    ev = sr.evaluate(X, D, got["H"], pin, components)
    M = sr._sets(k, pin, components)
    assert got["converged"].all() and got["nonfinite"] == 0
    slack = 1e-9 * np.maximum(1.0, ev["scale"])
    assert (got["gap"] <= TOL).all() and (ev["gap"] <= TOL + slack).all()
    assert (np.abs(got["gap"] - ev["gap"]) <= slack).all()
    assert (np.abs(got["deviance"] - ev["deviance"]) <= 1e-9 * np.abs(ev["deviance"])).all()
    if M.any():   # (an empty set holds no sum)
        assert (np.abs(ev["sum"] - ev["total"]) <= sr.sum_bound(k, ev["total"])).all()
    rest = ~M
    if pin is not None:
        # 2 (g_pin - lin / total): lin / total is an average of the g_j with the weights h_j / total (at total == 0: gmin itself)
        assert (np.abs(got["slope"] - ev["slope"]) <= 4.0 * slack).all()
        assert np.array_equal(got["H"][pin], np.broadcast_to(t, got["H"][pin].shape))   # bit for bit
        rest[pin] = False
    assert not got["H"][rest].any() and (got["H"] >= 0).all() and np.isfinite(got["H"]).all()
    return ev


# ---- solver-agnostic correctness of every fit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", POINTS)
@pytest.mark.parametrize("name", sr.CASES)
def test_fit_recomputed_in_numpy(presence, name, label):
    X, D = sr.case(name)
    if label != "full" and D.shape[1] == 1:   # one component: nothing beside the pinned one
        got = _unmix(X, D, 0, 0.5, None, components=[])
        _certified(X, D, got, 0, 0.5, [])
        assert not got["n_pass"].any() and not got["gap"].any()
        return
    got, ref, opt = _fitted(name, label), _reference(name, label), _reference(name, label, 1e-10)
    assert got["H"].shape == (D.shape[1], X.shape[1]) and got["converged"].dtype == bool
    n = got["n_pass"]
    print(f"{name} {label}: passes max {n.max()} (reference {ref['n_pass'].max()}), sum {n.sum()} (reference {ref['n_pass'].sum()}); "
          f"dev - dev_opt <= {np.max(got['deviance'] - opt['deviance']):.3g}")
    if label == "full":
        _certified(X, D, got)
    else:
        _certified(X, D, got, _pin(name), sr.pins(name)[label])
    assert opt["converged"].all() and (got["deviance"] <= opt["deviance"] + TOL).all()
    assert n.sum() <= 1.25 * ref["n_pass"].sum() and n.max() <= sr.MAX_PASS // 2


def test_a_component_subset_a_scalar_value_and_a_given_start(presence):
    X, D = sr.case("low8")
    comp, pin = [1, 4, 6], 3
    got = _unmix(X, D, pin, 0.25, None, components=comp)
    _certified(X, D, got, pin, 0.25, comp)
    opt = sr.ml_unmix(X, D, None, comp, pin, 0.25, 1e-10, 20000)
    assert opt["converged"].all() and (got["deviance"] <= opt["deviance"] + TOL).all()
    assert _same(_unmix(np.ascontiguousarray(X.T), D, pin, np.full(X.shape[1], 0.25), None, "pm", components=comp), got)
    # the full fit over a subset, from a start with zeros and the wrong scale: lifted and brought onto the simplex
    H0 = np.array(sr.solved("low8")["H"]) * 37.0
    H0[4, ::2] = 0.0
    sub = _full(X, D, H0, components=comp)
    _certified(X, D, sub, None, None, comp)
    opt = sr.ml_unmix(X, D, None, comp, None, None, 1e-10, 20000)
    assert (sub["deviance"] <= opt["deviance"] + TOL).all()


# ---- what is promised bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ("full", "mid"))
@pytest.mark.parametrize("name", BITS)
def test_both_layouts_and_every_dtype_give_the_same_bits(presence, name, label):
    X = sr.case(name)[0]
    want = _fitted(name, label)
    assert _same(_fitted(name, label, "pm"), want)
    for dtype in (np.uint16, np.float32, np.float64):
        assert _same(_run(name, label, X.astype(dtype)), want), dtype
        assert _same(_run(name, label, np.ascontiguousarray(X.T).astype(dtype), "pm"), want), dtype


@pytest.mark.parametrize("label", ("full", "mid"))
@pytest.mark.parametrize("name", BITS)
def test_the_split_into_calls_does_not_matter(presence, name, label):
    want = _fitted(name, label)   # (chunk = 64)
    assert want["n_pass"].max() >= 2   # (more than one chunk of 1)
    for chunk in (1, 7):
        assert _same(_run(name, label, chunk=chunk), want), chunk


@pytest.mark.parametrize("name", BITS)
def test_padded_rows_and_two_slabs(presence, name):
    import torch
    X, D = sr.case(name)
    pin, t, H0, want, full = _pin(name), sr.pins(name)["mid"], sr.solved(name)["H"], _fitted(name, "mid"), _fitted(name, "full")
    p = X.shape[1]
    for layout, Xl in (("cm", X), ("pm", np.ascontiguousarray(X.T))):
        wide = torch.zeros((Xl.shape[0], Xl.shape[1] + 13), dtype=torch.uint8, device="cuda")
        wide[:, :Xl.shape[1]] = torch.from_numpy(np.array(Xl)).cuda()
        view = wide[:, :Xl.shape[1]]
        assert view.stride(0) == Xl.shape[1] + 13
        assert _same(_run(name, "mid", view, layout), want), layout
        assert _same(_run(name, "full", view, layout), full), layout
    # two slabs against one call: an odd cut, t sliced with the pixels, the second slab a view into the whole image on the device
    cut = p // 3 | 1
    whole = torch.from_numpy(np.array(X)).cuda()
    first = _unmix(np.ascontiguousarray(X[:, :cut]), D, pin, t[:cut], H0[:, :cut])
    second = _unmix(whole[:, cut:], D, pin, t[cut:], H0[:, cut:])
    assert all(np.array_equal(np.concatenate([first[k], second[k]], axis=-1), want[k]) for k in PKEYS)
    pm = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    assert all(np.array_equal(_unmix(pm[cut:], D, pin, t[cut:], H0[:, cut:], "pm")[k], want[k][..., cut:]) for k in PKEYS)
    assert all(np.array_equal(_full(whole[:, cut:], D)[k], full[k][..., cut:]) for k in KEYS)


# ---- the state rules, through the entry point itself --------------------------------------------------------------------------------------
class _Raw:
    """The entry point on device tensors of the caller: the state is in plain sight, and every output starts as garbage."""

    def __init__(self, name, label="mid", pinned=True):
        import torch

        from espm_amd import _lib
        X, D = sr.case(name)
        self.n, self.p, self.k = X.shape[0], X.shape[1], D.shape[1]
        self.pin = self.k - 1 if pinned else -1
        self.s = np.ascontiguousarray(D.sum(axis=0))
        self.X, self.D = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(D)).cuda()
        self.H = torch.from_numpy(np.ascontiguousarray(sr.pp.start_from(X, D))).cuda()
        self.t = torch.from_numpy(np.ascontiguousarray(sr.pins(name)[label])).cuda()
        self.dev, self.gap, self.slope = (torch.full((self.p,), -7.0, dtype=torch.float64, device="cuda") for _ in range(3))
        self.passes = torch.zeros(self.p, dtype=torch.int32, device="cuda")
        self.done = torch.zeros(self.p, dtype=torch.uint8, device="cuda")
        self.counters = torch.zeros(3, dtype=torch.int64, device="cuda")
        self.extra = torch.full((self.k + _lib.PMLN_STATE_EXTRA, self.p), float("nan"), dtype=torch.float64, device="cuda")   # (never read before written)

    def call(self, n_pass, tol=TOL):
        from espm_amd import _lib
        from espm_amd.engine import _ptr, _stream
        mask = (1 << self.k) - 1
        if self.pin >= 0:
            mask &= ~(1 << self.pin)
        t, slope = (_ptr(self.t), _ptr(self.slope)) if self.pin >= 0 else (None, None)   # (nothing pinned: neither is needed)
        rc = _lib.lib.espm_pixel_ml_simplex(_ptr(self.X), _lib.DIAG_X_U8, _lib.LAYOUT_CM, self.p, self.n, self.p, _ptr(self.D),
                                            self.s.ctypes.data_as(C.c_void_p), self.k, mask, self.pin, t, 1e-14, tol, n_pass,
                                            _ptr(self.H), _ptr(self.dev), _ptr(self.gap), slope, _ptr(self.passes), _ptr(self.done),
                                            _ptr(self.counters), _ptr(self.extra), self.extra.numel() * 8, _stream())
        _lib.check(rc)
        return self

    def state(self):
        return tuple(t.cpu().numpy().copy() for t in (self.H, self.dev, self.gap, self.slope, self.passes, self.done, self.counters, self.extra))


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "free"])
def test_resumable_garbage_state_and_a_done_pixel_is_never_touched(presence, pinned):
    a, b = 3, 4
    one = _Raw("planted", pinned=pinned).call(a + b).state()
    two = _Raw("planted", pinned=pinned).call(a)
    mid = two.state()
    then = two.call(b).state()
    # a + b passes: the bits of one call, counters included; the state (NaN before the first call) compares equal where it was written
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(one, then))
    assert np.isfinite(then[0]).all() and np.isfinite(then[1]).all() and np.isfinite(then[2]).all()
    assert np.isfinite(then[3]).all() and (pinned or (then[3] == -7.0).all())   # (no pinned component: slope is never written)
    done_mid = mid[5] == 1
    assert 0 < done_mid.sum() < done_mid.size and 0 < (then[5] == 1).sum() < done_mid.size   # (some done after a, not all after a + b)
    assert then[6][0] == (then[5] == 0).sum() and mid[6][0] == (mid[5] == 0).sum()           # the one integer the host loop reads
    for u, v in zip(mid[:6], then[:6]):
        assert np.array_equal(u[..., done_mid], v[..., done_mid])
    left = then[5] == 0
    assert (then[4][left] == a + b).all() and (then[2][left] > TOL).all() and (then[2][then[5] == 1] <= TOL).all()
    assert (then[1][left] <= mid[1][left]).all()   # a pixel still running reports its last ACCEPTED point
    # pixels the caller retired before the first call: everything of theirs keeps its bits, garbage included
    raw = _Raw("planted", pinned=pinned)
    raw.done[::3] = 1
    before = raw.state()
    after = raw.call(sr.MAX_PASS).state()
    gone = before[5] == 1
    for u, v in zip(before[:6] + before[7:], after[:6] + after[7:]):
        assert np.array_equal(u[..., gone], v[..., gone], equal_nan=True)
    assert (after[5][~gone] == 1).all() and after[6][0] == 0
    full = _Raw("planted", pinned=pinned).call(sr.MAX_PASS).state()
    for u, v in zip(full[:5], after[:5]):   # ... and the others do not notice
        assert np.array_equal(u[..., ~gone], v[..., ~gone])
    # all done: a further call writes nothing at all
    raw.H += 1.0
    again = raw.call(50).state()
    assert np.array_equal(again[0], after[0] + 1.0) and all(np.array_equal(u, v, equal_nan=True) for u, v in zip(after[1:], again[1:]))


def test_a_value_of_one_above_one_and_not_finite(presence):
    raw = _Raw("planted")
    raw.t[2] = 1.0
    raw.t[3], raw.t[7], raw.t[11], raw.t[13] = -1.0, float("nan"), float("inf"), 1.0 + 1e-12
    H0 = raw.H.cpu().numpy().copy()
    out = raw.call(sr.MAX_PASS).state()
    bad = np.zeros(raw.p, dtype=bool)
    bad[[3, 7, 11, 13]] = True
    assert (out[5][bad] == 2).all() and (out[5][~bad] == 1).all() and out[6][2] == 4 and out[6][0] == 0
    assert np.array_equal(out[0][:, bad], H0[:, bad]) and not out[4][bad].any()
    assert not out[1][bad].any() and not out[2][bad].any() and not out[3][bad].any()
    # t = 1: nothing is left for the others; done in the first pass, the slope 2 (g_pin - gmin)
    assert out[0][-1, 2] == 1.0 and not out[0][:-1, 2].any() and out[4][2] == 0 and out[2][2] == 0
    X, D = sr.case("planted")
    ev = sr.evaluate(X[:, ~bad], D, out[0][:, ~bad], raw.k - 1)
    assert abs(out[3][2] - ev["slope"][2]) <= 1e-9 * ev["scale"][2] and abs(out[1][2] - ev["deviance"][2]) <= 1e-9 * ev["deviance"][2]
    # through the Python layer: every pixel at t = 1
    top = _fitted("planted", "one")
    assert (top["H"][-1] == 1).all() and not top["H"][:-1].any() and not top["n_pass"].any() and not top["gap"].any()


def test_the_special_pixels(presence):
    """The empty pixel and the pixel whose counts no component reaches: the vertex of the least s (the lowest index on ties), one
    pass, gap exactly 0.  One component in the set: h = 1 and no pass.  One component in all: the same."""
    X, D = sr.case("zero_row")
    got, ref = _fitted("zero_row", "full"), sr.solved("zero_row")
    best = int(np.argmin(D.sum(axis=0)))
    want = np.zeros(D.shape[1])
    want[best] = 1.0
    for q in (5, X.shape[1] - 1):
        assert np.array_equal(got["H"][:, q], want) and got["gap"][q] == 0 and got["n_pass"][q] == 1 and got["converged"][q]
        assert abs(got["deviance"][q] - ref["deviance"][q]) <= 1e-9 * ref["deviance"][q]
    assert got["unmodelled"] == ref["unmodelled"] == 1
    # pinned, too (from the even start: far enough from the vertex not to certify at once): the others' share goes to the vertex of
    # the least s among them
    t = sr.pins("zero_row")["mid"]
    pin = _unmix(X, D, D.shape[1] - 1, t, None)
    _certified(X, D, pin, D.shape[1] - 1, t)
    rest_best = int(np.argmin(D.sum(axis=0)[:-1]))
    for q in (5, X.shape[1] - 1):
        assert pin["H"][rest_best, q] == 1.0 - t[q] and pin["H"][-1, q] == t[q] and pin["gap"][q] == 0 and pin["n_pass"][q] == 1
        assert not np.delete(pin["H"][:, q], [rest_best, D.shape[1] - 1]).any()
    one = _full(X, D, components=[2])
    assert (one["H"][2] == 1).all() and not np.delete(one["H"], 2, axis=0).any() and not one["n_pass"].any() and (one["gap"] == 0).all()
    assert one["converged"].all()
    ev = sr.evaluate(X, D, one["H"], None, [2])
    assert (np.abs(one["deviance"] - ev["deviance"]) <= 1e-9 * ev["deviance"]).all()
    k1 = _fitted("img96_k1", "full")
    assert (k1["H"] == 1).all() and not k1["n_pass"].any() and (k1["gap"] == 0).all() and k1["converged"].all()
    # one fitted component beside a pinned one: h = 1 - t exactly, gap exactly 0
    two = _unmix(X, D, 0, 0.3, None, components=[3])
    assert (two["H"][3] == 1.0 - 0.3).all() and (two["H"][0] == 0.3).all() and not two["n_pass"].any() and (two["gap"] == 0).all()


# ---- presence -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("planted", "low8", "img96_k5", "dim03", "zero_row"))
def test_presence_against_the_reference(presence, name):
    """Each of the two deviances behind an lr is within its gap <= tol above the same minimum on the device and in the reference:
    the two statistics differ by at most 2 tol.  Exactly 0 wherever the full fit has h_j == 0: the zeros of a vertex (``zero_row``: the
    empty pixel and the pixel whose counts nothing reaches), where the fit without j finds the same vertex."""
    X, D = sr.case(name)
    k, p = D.shape[1], X.shape[1]
    got, ref = presence.presence(X, D, tol=TOL, max_pass=sr.MAX_PASS, method="simplex"), sr.presence_solved(name)
    assert got["lr"].shape == got["pvalue"].shape == (k, p) and got["converged"].shape == got["gap"].shape == got["n_pass"].shape == (k + 1, p)
    assert got["converged"].all() and (got["gap"] <= TOL).all() and got["nonfinite"] == 0
    print(f"{name}: |lr - reference| <= {np.abs(got['lr'] - ref['lr']).max():.3g}; passes {got['n_pass'].sum()} (reference {ref['n_pass'].sum()})")
    assert (np.abs(got["lr"] - ref["lr"]) <= 2 * TOL).all()
    assert got["n_pass"].sum() <= 1.25 * ref["n_pass"].sum() and got["n_pass"].max() <= sr.MAX_PASS // 2
    gone = got["H_ml"] == 0
    assert (got["lr"][gone] == 0).all() and (got["pvalue"][gone] == 1).all()
    assert (np.abs(got["H_ml"].sum(axis=0) - 1.0) <= sr.sum_bound(k, 1.0)).all()
    assert np.array_equal(got["H_ml"], _fitted(name, "full")["H"])
    if name == "zero_row":
        assert gone[:, 5].sum() == 3 and gone[:, -1].sum() == 3
    if name == "planted":
        pm = presence.presence(np.ascontiguousarray(X.T), D, tol=TOL, max_pass=sr.MAX_PASS, method="simplex", layout="pm")
        assert all(np.array_equal(pm[key], got[key]) for key in ("H_ml", "deviance_ml", "lr", "pvalue", "converged", "gap", "n_pass"))


# ---- intervals ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _intervals(name, layout="cm"):
    from espm_amd import presence
    X, D = sr.case(name)
    return presence.intervals(X if layout == "cm" else np.ascontiguousarray(X.T), D, max_pass=sr.MAX_PASS, layout=layout, simplex=True)


@pytest.mark.parametrize("name", sr.CASES)
def test_interval_ends_against_the_long_runs(presence, name):
    """|g*(t) - dev* - q| <= lr_tol + tol + 1e-9 dev* at every end the root finder placed: each reported deviance lies within its
    gap <= tol above its minimum, and the stop is lr_tol on the reported values.  An end at exactly 0 or exactly 1 is a boundary:
    there the profile has not reached the level, g*(t) - dev* - q <= the same bound."""
    X, D = sr.case(name)
    k, p = D.shape[1], X.shape[1]
    got, ref, q = _intervals(name), sr.intervals_solved(name), sr.threshold(0.95)
    assert got["lower"].shape == got["upper"].shape == (k, p) and got["converged"].shape == got["n_eval"].shape == got["n_pass"].shape == (k, 2, p)
    assert got["converged"].dtype == bool and got["level"] == 0.95 and abs(got["threshold"] - q) <= 1e-12 and got["nonfinite"] == 0
    print(f"{name}: evaluations per end <= {got['n_eval'].max()} (reference {ref['n_eval'].max()}), passes {got['n_pass'].sum()} "
          f"(reference {ref['n_pass'].sum()}); lower == 0 in {np.mean(got['lower'] == 0):.3f} of the entries, upper == 1 in "
          f"{np.mean(got['upper'] == 1):.3f}")
    assert got["converged"].all() and np.isfinite(got["lower"]).all() and np.isfinite(got["upper"]).all()
    assert got["n_eval"].max() <= 32 and got["n_pass"].sum() <= 1.25 * ref["n_pass"].sum()
    assert (0 <= got["lower"]).all() and (got["lower"] <= got["H_ml"]).all() and (got["H_ml"] <= got["upper"]).all() and (got["upper"] <= 1).all()
    assert np.array_equal(got["H_ml"], _fitted(name, "full")["H"])
    dev_opt = sr.solved(name, 1e-10)["deviance"]
    bound = LR_TOL + TOL + 1e-9 * dev_opt
    worst = 0.0
    for j in range(k):
        rest = [i for i in range(k) if i != j]
        for side, end in ((0, got["lower"][j]), (1, got["upper"][j])):
            opt = sr.ml_unmix(X, D, got["H_ml"], rest, j, end, 1e-10, 20000)
            assert opt["converged"].all()
            phi = opt["deviance"] - dev_opt - q
            edge = (end == 0) if side == 0 else (end == 1)
            worst = max(worst, float(np.abs(phi[~edge]).max(initial=0.0)))
            assert (np.abs(phi[~edge]) <= bound[~edge]).all(), (j, side)
            assert (phi[edge] <= bound[edge]).all(), (j, side)
    print(f"{name}: |g*(t) - dev* - q| <= {worst:.3g}")


def test_the_cap_the_boundary_and_the_layout(presence):
    X, D = sr.case("planted")
    got, q = _intervals("planted"), sr.threshold(0.95)
    assert (got["upper"] == 1).any()   # a pixel that could be all one phase: the upper end is the cap, exactly
    assert not X[:, 5].any() and (got["lower"][:, 5] == 0).all() and np.isfinite(got["upper"][:, 5]).all()   # the empty pixel: the general path
    lr = presence.presence(X, D, tol=TOL, max_pass=sr.MAX_PASS, method="simplex")["lr"]
    clear = np.abs(lr - q) > 2 * TOL
    print(f"planted: lr <= q in {np.mean(lr <= q):.3f} of the entries, {np.sum(~clear)} within 2 tol of q")
    assert np.array_equal((got["lower"] == 0)[clear], (lr <= q)[clear])
    pm = _intervals("planted", "pm")
    assert all(np.array_equal(pm[key], got[key]) for key in ("H_ml", "deviance_ml", "lower", "upper", "converged", "n_eval", "n_pass"))
    # one component: h = 1, the upper end is the cap without an evaluation
    one = _intervals("img96_k1")
    assert (one["H_ml"] == 1).all() and (one["upper"] == 1).all() and not one["n_eval"][:, 1].any() and one["converged"].all()
    # a subset of the rows: the others stay NaN, the row itself does not notice
    sub = presence.intervals(X, D, components=[1], max_pass=sr.MAX_PASS, simplex=True)
    for key in ("lower", "upper"):
        assert np.isnan(np.delete(sub[key], 1, axis=0)).all() and np.array_equal(sub[key][1], got[key][1])


# ---- the estimator and the adapter --------------------------------------------------------------------------------------------------------
SHAPE = (15, 20)
KEPT = ("W_", "H_", "G_")


def _fit(hspy_comp=False, simplex_H=True):
    from espm_amd.estimators import SmoothNMF
    X = sr.case("planted")[0]
    est = SmoothNMF(n_components=3, max_iter=200, tol=0.0, verbose=0, random_state=0, shape_2d=SHAPE, simplex_H=simplex_H, simplex_W=False,
                    hspy_comp=hspy_comp)
    Xin = np.ascontiguousarray(X.T) if hspy_comp else X
    est.fit(Xin.astype(np.float32))
    return est, Xin


@pytest.mark.parametrize("hspy_comp", [False, True], ids=["cm", "hspy"])
def test_estimator_and_adapter(presence, hspy_comp):
    from espm_amd import hyperspy_adapter as ha
    est, Xin = _fit(hspy_comp)
    kept = {a: np.array(getattr(est, a)) for a in KEPT if getattr(est, a, None) is not None}
    k, p = 3, 300
    layout = "pm" if hspy_comp else "cm"
    G, W, _ = est._model_factors()
    D = W if G is None else G @ W
    H = np.asarray(est.H_, dtype=np.float64)
    # presence maps under the simplex
    out = est.presence_maps(X=Xin, max_pass=sr.MAX_PASS, method="simplex")
    assert est.ml_method_ == "simplex" and est.H_ml_.shape == est.presence_lr_.shape == est.presence_pvalue_.shape == (k, p)
    assert est.ml_converged_.shape == est.ml_gap_.shape == est.ml_n_pass_.shape == (k + 1, p) and est.ml_converged_.all()
    assert (np.abs(est.H_ml_.sum(axis=0) - 1.0) <= sr.sum_bound(k, 1.0)).all() and out["H_ml"].shape == ((p, k) if hspy_comp else (k, p))
    want = presence.presence(Xin, D, H, max_pass=sr.MAX_PASS, log_shift=est.log_shift, layout=layout, method="simplex")
    assert np.array_equal(want["lr"], est.presence_lr_) and np.array_equal(want["H_ml"], est.H_ml_)
    # the fit's own H is a point of the simplex: the constrained ML is not above it (+ tol)
    Xcm = Xin.T if hspy_comp else Xin
    assert (est.deviance_ml_ <= sr.evaluate(Xcm, D, H / H.sum(axis=0), log_shift=est.log_shift)["deviance"] + TOL).all()
    maps = ha.presence_maps(est)
    assert maps[0].shape == (k,) + SHAPE and np.array_equal(maps[1].reshape(k, p), est.presence_lr_)
    # intervals under the simplex
    out = est.abundance_intervals(X=Xin, simplex=True)
    assert est.H_interval_simplex_ is True and est.H_interval_level_ == 0.95
    assert est.H_lower_.shape == est.H_upper_.shape == est.H_ml_.shape == (k, p) and est.deviance_ml_.shape == (p,)
    assert est.H_interval_converged_.shape == est.H_interval_n_eval_.shape == (k, 2, p) and est.H_interval_converged_.all()
    assert (0 <= est.H_lower_).all() and (est.H_lower_ <= est.H_ml_).all() and (est.H_ml_ <= est.H_upper_).all() and (est.H_upper_ <= 1).all()
    shape = (p, k) if hspy_comp else (k, p)
    assert out["H_ml"].shape == out["lower"].shape == out["upper"].shape == shape
    assert np.array_equal(out["upper"].T if hspy_comp else out["upper"], est.H_upper_)
    want = presence.intervals(Xin, D, H, log_shift=est.log_shift, layout=layout, simplex=True)
    assert np.array_equal(want["lower"], est.H_lower_) and np.array_equal(want["upper"], est.H_upper_)
    lo, up = ha.abundance_interval_maps(est)
    assert lo.shape == up.shape == (k,) + SHAPE and np.array_equal(up.reshape(k, p), est.H_upper_)
    for a, v in kept.items():
        assert np.array_equal(np.asarray(getattr(est, a)), v), a
    # the defaults are what they were: the free-scale interval, and the flag says so
    est.abundance_intervals(X=Xin, components=[2])
    assert est.H_interval_simplex_ is False


def test_estimator_and_adapter_refuse_a_fit_without_the_simplex(presence):
    from espm_amd import hyperspy_adapter as ha
    est, Xin = _fit(simplex_H=False)
    with pytest.raises(ValueError, match="simplex_H"):
        est.presence_maps(X=Xin, method="simplex")
    with pytest.raises(ValueError, match="simplex_H"):
        est.abundance_intervals(X=Xin, simplex=True)
    with pytest.raises(ValueError, match="simplex_H"):
        ha.presence_maps(est, method="simplex")
    assert not hasattr(est, "ml_method_") and not hasattr(est, "H_interval_simplex_")
