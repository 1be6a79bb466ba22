"""Channel ML on the device: the step kernel alone (csrc/mu_channel_ml.hip, espm_channel_ml_step) on hand-made sums against the numpy
rule, ``channel_ml.ml_channels``, ``presence``, ``ml_channels_pinned`` and ``intervals`` against the numpy definition of
tests/channel_ml_reference.py (the pixel rules on (X^T, H^T)), what the lockstep promises bit for bit, and
``est.spectrum_presence`` / ``est.spectrum_intervals``.  tests/test_channel_ml_cpu.py holds what this rests on: the reference alone
converges on every channel of every case within half of the caps passed here, so ``converged`` is required everywhere.

The checks of the fits are SOLVER-AGNOSTIC: a returned point is held against long runs of the numpy rule (tol = 1e-10 for the full
fit, 1e-8 for a pinned one) with the bounds that follow from the certificates; nothing compares the paths."""
import ctypes as C
import functools

import numpy as np
import pytest

import channel_ml_reference as R
import pixel_ml_newton_reference as nr
from test_gpu_pixel_diagnostics import quiet

pytestmark = pytest.mark.gpu

TOL, LR_TOL = 1e-3, 1e-2
MULTI = ("A", "B", "C8")   # the cases with more than one component


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def cml(lib):
    from espm_amd import channel_ml
    return channel_ml


@functools.lru_cache(maxsize=None)
def _full(name):
    from espm_amd import channel_ml
    X, H, _ = R.case(name)
    return channel_ml.ml_channels(X, H, max_pass=R.MAX_PASS)


@functools.lru_cache(maxsize=None)
def _presence(name):
    from espm_amd import channel_ml
    X, H, _ = R.case(name)
    return channel_ml.presence(X, H, max_pass=R.MAX_PASS)


@functools.lru_cache(maxsize=None)
def _intervals(name):
    from espm_amd import channel_ml
    X, H, _ = R.case(name)
    return channel_ml.intervals(X, H, max_pass=R.MAX_PASS, max_eval=R.MAX_EVAL)


def _slack(dev):
    """The rounding allowance of a deviance held against another one (tests/test_spectra_ml_cpu.py's)."""
    return 1e-9 * np.maximum(1.0, np.abs(dev))


# ---- the step kernel alone, on hand-made sums -------------------------------------------------------------------------------------------------
def _sums(X, H, d, log_shift=R.LOG_SHIFT):
    """What espm_spectra_ml_pass_batch delivers at the model d (n, k), in numpy: dev (n,), q (n, k), the triangle (n, k (k + 1) / 2)."""
    x = np.asarray(X, dtype=np.float64)
    Y = d @ H
    Y = np.where(Y >= log_shift, Y, log_shift)
    w = x * (1.0 / Y)
    t = Y - x
    pos = x > 0
    t[pos] += x[pos] * np.log(w[pos])
    A = np.einsum("cp,jp,lp->cjl", w * (1.0 / Y), H, H)
    il, jl = np.tril_indices(H.shape[0])
    return 2.0 * t.sum(axis=1), w @ H.T, np.ascontiguousarray(A[:, il, jl])


def _tri_to_full(tri, k):
    il, jl = np.tril_indices(k)
    A = np.zeros(tri.shape[:-1] + (k, k))
    A[..., il, jl] = tri
    A[..., jl, il] = tri
    return A


def _rule_step(h, q, tri, s, N, M, pin, tau, free):
    """The numpy rule's step of an ACCEPTED point h (n, k) that does not stop: (the next point, its EM successor e, bad (n,))."""
    k = h.shape[1]
    A = _tri_to_full(tri, k)
    idx = np.flatnonzero(M)
    hM, qM, sM = h[:, idx], q[:, idx], s[idx]
    e = h.copy()
    e[:, idx] = hM * (qM / sM)
    B = A[:, idx][:, :, idx].copy()
    with np.errstate(all="ignore"):
        B[:, np.arange(idx.size), np.arange(idx.size)] += tau[:, None] * (sM[None, :] / hM)
        delta, bad = nr._solve(B, sM[None, :] - qM)
        new = np.maximum(np.maximum(hM + delta, nr.THETA * hM), nr.H_FLOOR * N[:, None] / sM[None, :])
    nxt = h.copy()
    nxt[:, idx] = np.where(bad[:, None], e[:, idx], new)
    return (_onto_ray(nxt, s, N, M) if free else nxt), e, bad


def _onto_ray(h, s, N, M):
    with np.errstate(all="ignore"):
        return h * (N / (h[:, M] @ s[M]))[:, None]


class _Raw:
    """espm_channel_ml_step by hand for the models ``pins`` of one image: every array the entry point reads or writes, on the device."""

    def __init__(self, X, H, pins, d0, t=None, mask=None, tol=TOL):
        import torch
        from espm_amd import _lib
        self.X, self.H = np.asarray(X, dtype=np.float64), np.asarray(H, dtype=np.float64)
        self.n, self.k, self.B = X.shape[0], H.shape[0], len(pins)
        n, k, B = self.n, self.k, self.B
        nt = k * (k + 1) // 2
        self.pins = np.ascontiguousarray(pins, dtype=np.int32)
        self.s = np.ascontiguousarray(self.H.sum(axis=1))
        self.N = self.X.sum(axis=1)
        self.mask = (1 << k) - 1 if mask is None else mask
        self.tol = tol
        f = dict(dtype=torch.float64, device="cuda")
        self.xsum = torch.from_numpy(self.N.copy()).cuda()
        self.d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(d0, (B, n, k)), dtype=np.float64)).cuda()
        self.t = None if t is None else torch.from_numpy(np.ascontiguousarray(np.broadcast_to(t, (B, n)), dtype=np.float64)).cuda()
        self.dev_in, self.q, self.tri = torch.zeros((B, n), **f), torch.zeros((B, n, k), **f), torch.zeros((B, n, nt), **f)
        self.state = torch.full((B, 2 * k + _lib.CML_STATE_EXTRA, n), float("nan"), **f)   # (never read before written)
        self.dev, self.gap, self.slope = (torch.full((B, n), -7.0, **f) for _ in range(3))
        self.passes = torch.full((B, n), 99, dtype=torch.int32, device="cuda")
        self.done = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
        self.active = torch.full((B,), 9, dtype=torch.uint8, device="cuda")
        self.live = torch.full((B,), 99, dtype=torch.int64, device="cuda")

    def call(self, start, **over):
        import torch
        from espm_amd import _lib
        from espm_amd.engine import _ptr, _stream
        a = dict(n=self.n, k=self.k, n_models=self.B, start=start, dev_in=_ptr(self.dev_in), q=_ptr(self.q), a_tri=_ptr(self.tri),
                 xsum=_ptr(self.xsum), s=self.s.ctypes.data_as(C.c_void_p), mask=self.mask, pin=self.pins.ctypes.data_as(C.c_void_p),
                 t=None if self.t is None else _ptr(self.t), tol=self.tol, d=_ptr(self.d), state=_ptr(self.state),
                 state_bytes=self.state.numel() * 8, dev=_ptr(self.dev), gap=_ptr(self.gap), slope=_ptr(self.slope),
                 passes=_ptr(self.passes), done=_ptr(self.done), active=_ptr(self.active), live=_ptr(self.live), stream=_stream())
        a.update(over)
        rc = _lib.lib.espm_channel_ml_step(*a.values())
        torch.cuda.synchronize()
        return rc

    def feed(self, sums):
        """The sums of every model, a list of (dev, q, tri), onto the device."""
        import torch
        for b, (dv, q, tri) in enumerate(sums):
            self.dev_in[b], self.q[b], self.tri[b] = torch.from_numpy(dv).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(tri).cuda()

    def host(self):
        return {key: getattr(self, key).cpu().numpy().copy() for key in ("d", "state", "dev", "gap", "slope", "passes", "done", "active", "live")}


def _close(got, want, rel=1e-13):
    return (np.abs(got - want) <= rel * np.abs(want)).all()


def test_step_kernel_on_hand_made_sums(lib):
    """One start, one accepted pass, one rejected pass and one bad-pivot pass of a free-scale model and a pinned model side by side: the
    next point against the numpy rule's to 1e-13, and the bookkeeping exactly."""
    import torch
    X, H, D = R.case("A")
    n, k = X.shape[0], H.shape[0]
    s, N = H.sum(axis=1), X.sum(axis=1).astype(np.float64)
    rng = np.random.default_rng(8)
    d0 = rng.uniform(0.5, 1.5, (n, k)) * 0.02
    d0[3, 1], d0[7, 0] = 0.0, -1.0                     # starts that are not positive: the rule's fill
    tpin = np.full(n, 0.004)
    raw = _Raw(X, H, [-1, 2], d0, t=tpin)
    empty = N == 0
    Mf, Mp = np.ones(k, dtype=bool), np.array([True, True, False])
    # pass 0
    assert raw.call(1) == lib.OK
    got = raw.host()
    fill = N[:, None] / (3 * s[None, :]) * 1e-3
    want_f = _onto_ray(np.where(d0 > 0, d0, fill), s, N, Mf)
    want_f[empty] = 0.0
    want_p = np.where(d0 > 0, d0, N[:, None] / (2 * s[None, :]) * 1e-3)
    want_p[empty] = 0.0
    want_p[:, 2] = tpin
    assert _close(got["d"][0], want_f) and _close(got["d"][1], want_p) and np.array_equal(got["d"][1][:, 2], tpin)
    assert np.array_equal(got["done"][0], empty.astype(np.uint8)) and not got["done"][1].any()
    assert not got["passes"].any() and not got["dev"].any() and not got["gap"].any() and not got["slope"][1].any()
    assert (got["slope"][0] == -7.0).all()             # (a free model has no slope: never written)
    assert list(got["live"]) == [n - empty.sum(), n] and list(got["active"]) == [1, 1]
    assert np.array_equal(got["state"][:, :k], got["d"].transpose(0, 2, 1)) and not got["state"][:, k:2 * k].any()
    assert np.isinf(got["state"][:, 2 * k]).all() and (got["state"][:, 2 * k + 1] == 1e-2).all() and not got["state"][:, 2 * k + 2].any()
    # an accepted pass: the certificate, the step, the ray
    h = got["d"]
    sums = [_sums(X, H, h[b]) for b in range(2)]
    raw.feed(sums)
    assert raw.call(0) == lib.OK
    acc = raw.host()
    tau = np.full(n, 1e-2)
    live = ~empty
    want, e_acc = [None, None], [None, None]
    for b, (M, free) in enumerate(((Mf, True), (Mp, False))):
        dv, q, tri = sums[b]
        r = q[:, M] / s[M]
        if free:
            gap = 2.0 * N * (r.max(axis=1) - 1.0)
        else:
            gap = 2.0 * (((s[M] - q[:, M]) * h[b][:, M]).sum(axis=1) + N * np.maximum(r.max(axis=1) - 1.0, 0.0))
            assert _close(acc["slope"][b][live], (2.0 * (s[2] - q[:, 2]))[live], 1e-12)
        assert (gap[live] > TOL).all()                 # (far from the optimum: every live channel steps)
        assert np.array_equal(acc["dev"][b][live], dv[live]) and _close(acc["gap"][b][live], gap[live], 1e-11)
        want[b], e_acc[b], bad = _rule_step(h[b][live], q[live], tri[live], s, N[live], M, 2, tau[live], free)
        assert not bad.any() and _close(acc["d"][b][live], want[b])
        assert (acc["passes"][b][live] == 1).all() and not acc["done"][b][live].any()
        assert np.array_equal(acc["state"][b][:k].T[live], h[b][live])                              # the accepted point
        assert _close(acc["state"][b][k:2 * k].T[live][:, M], e_acc[b][:, M])                       # its EM successor
        assert np.array_equal(acc["state"][b][2 * k][live], dv[live]) and (acc["state"][b][2 * k + 2][live] == 1.0).all()
    # the empty channel: untouched under the free rule, done in its first pass under the pinned one (the closed form, no pass counted)
    assert np.array_equal(acc["d"][0][empty], got["d"][0][empty]) and (acc["passes"][0][empty] == 0).all()
    closed = 2.0 * np.maximum(tpin[empty][:, None] * H[2][None, :], R.LOG_SHIFT).sum(axis=1)
    assert (acc["done"][1][empty] == 1).all() and (acc["passes"][1][empty] == 0).all() and (acc["gap"][1][empty] == 0).all()
    assert _close(acc["dev"][1][empty], closed, 1e-12) and np.array_equal(acc["d"][1][empty], got["d"][1][empty])
    assert list(acc["live"]) == [live.sum(), live.sum()]
    # a rejected pass: the deviance of the trial made to rise by hand - back to the EM successor, a heavier blend, one pass more
    sums = []
    for b in range(2):
        _, q, tri = _sums(X, H, acc["d"][b])
        sums.append((acc["dev"][b] + 1.0, q, tri))
    raw.feed(sums)
    assert raw.call(0) == lib.OK
    rej = raw.host()
    for b, (M, free) in enumerate(((Mf, True), (Mp, False))):
        back = e_acc[b].copy()
        if free:
            back = _onto_ray(back, s, N[live], M)
        assert _close(rej["d"][b][live][:, M], back[:, M]) and np.array_equal(rej["d"][1][:, 2], tpin)
        assert (rej["passes"][b][live] == 2).all() and not rej["done"][b][live].any()
        assert np.array_equal(rej["dev"][b], acc["dev"][b]) and np.array_equal(rej["gap"][b], acc["gap"][b])
        assert np.array_equal(rej["state"][b][:2 * k + 1], acc["state"][b][:2 * k + 1])            # the accepted point, e and dev_acc stay
        assert _close(rej["state"][b][2 * k + 1][live], np.full(live.sum(), 0.1), 1e-15) and not rej["state"][b][2 * k + 2][live].any()
    # a bad-pivot pass: an information matrix that is none (its first diagonal entry hugely negative) - the EM successor instead
    h = rej["d"]
    sums = [_sums(X, H, h[b]) for b in range(2)]
    for sm in sums:
        sm[2][:, 0] = -1e300
    raw.feed(sums)
    assert raw.call(0) == lib.OK
    piv = raw.host()
    for b, (M, free) in enumerate(((Mf, True), (Mp, False))):
        dv, q, tri = sums[b]
        nxt, e, bad = _rule_step(h[b][live], q[live], tri[live], s, N[live], M, 2, np.full(live.sum(), 0.1), free)
        assert bad.all() and _close(piv["d"][b][live], nxt)
        assert (piv["passes"][b][live] == 3).all() and not piv["state"][b][2 * k + 2][live].any()
        assert np.array_equal(piv["state"][b][2 * k + 1][live], rej["state"][b][2 * k + 1][live])   # (no trial before: tau stays)
    # a problem that is done is bit-untouched by further calls, whatever the sums hold
    raw.done[:] = 1
    raw.done[1, 4] = 0
    before = raw.host()
    raw.dev_in[:], raw.q[:], raw.tri[:] = float("nan"), float("nan"), float("nan")
    raw.q[1, 4], raw.tri[1, 4], raw.dev_in[1, 4] = torch.from_numpy(s).cuda(), 0.0, 5.0     # q = s: the gradient vanishes, gap 0
    assert raw.call(0) == lib.OK
    after = raw.host()
    keep = np.ones((2, n), dtype=bool)
    keep[1, 4] = False
    for key in ("d", "dev", "gap", "slope", "passes", "done"):
        assert np.array_equal(after[key][keep], before[key][keep], equal_nan=True), key
    assert np.array_equal(after["state"].transpose(0, 2, 1)[keep], before["state"].transpose(0, 2, 1)[keep], equal_nan=True)
    assert list(after["live"]) == [0, 0] and list(after["active"]) == [0, 0] and after["done"][1, 4] == 1 and after["dev"][1, 4] == 5.0


def test_step_kernel_lines(cml):
    """The empty channel, one component, a one-component mask and a pinned value that is none, each against the definition."""
    X, H, _ = R.case("A")
    full = _full("A")
    empty = full["N"] == 0
    assert empty.sum() == 1 and not full["D"][empty].any() and (full["deviance"][empty] == 0).all() and (full["n_pass"][empty] == 0).all()
    assert full["converged"][empty].all() and (full["gap"][empty] == 0).all()
    X1, H1, _ = R.case("C1")
    one, ref = _full("C1"), R.ml_channels(X1, H1)
    assert one["converged"].all() and not one["n_pass"].any() and _close(one["D"], ref["D"], 1e-13) and (np.abs(one["gap"]) <= TOL).all()
    masked, ref = cml.ml_channels(X, H, components=[1]), R.ml_channels(X, H, components=[1])
    assert masked["converged"].all() and not masked["n_pass"].any() and not masked["D"][:, [0, 2]].any() and _close(masked["D"], ref["D"], 1e-13)
    assert _close(masked["deviance"], ref["deviance"], 1e-11)
    t = np.full(X.shape[0], 0.01)
    t[2], t[11] = -1e-3, np.nan
    pinned = cml.ml_channels_pinned(X, H, 0, t, max_pass=R.MAX_PASS)
    good = np.ones(X.shape[0], dtype=bool)
    good[[2, 11]] = False
    assert pinned["nonfinite"] == 2 and not pinned["converged"][~good].any() and pinned["converged"][good].all()
    assert not pinned["n_pass"][~good].any() and not pinned["deviance"][~good].any()
    alone = cml.ml_channels_pinned(X, H, 0, 0.01, components=[], max_pass=R.MAX_PASS)     # nothing fitted: one evaluating pass, gap 0
    assert alone["converged"].all() and not alone["n_pass"].any() and not alone["gap"].any() and not alone["D"][:, 1:].any()
    assert _close(alone["deviance"], R.ml_channels_pinned(X, H, 0, 0.01, components=[])["deviance"], 1e-11)


def test_step_kernel_refusals(lib):
    X, H, _ = R.case("A")
    n, k = X.shape[0], H.shape[0]
    raw = _Raw(X, H, [-1, 1], np.full((n, k), 0.01), t=np.zeros(n))
    bad = [dict(n=0), dict(n_models=0), dict(n_models=65536), dict(mask=0), dict(mask=0b1111), dict(tol=0.0), dict(tol=float("nan")),
           dict(xsum=None), dict(s=None), dict(pin=None), dict(d=None), dict(state=None), dict(dev=None), dict(gap=None), dict(passes=None),
           dict(done=None), dict(active=None), dict(live=None), dict(t=None), dict(slope=None), dict(state_bytes=raw.state.numel() * 8 - 1),
           dict(start=0, dev_in=None), dict(start=0, q=None), dict(start=0, a_tri=None), dict(mask=0b101)]    # (pin 1 outside the mask)
    for over in bad:
        before = raw.host()
        assert raw.call(over.pop("start", 1), **over) == lib.EINVAL, over
        assert lib.last_error().startswith("channel ML step:")
        after = raw.host()
        assert all(np.array_equal(before[key], after[key], equal_nan=True) for key in before), over   # nothing was launched
    for pins in ([-2, 1], [3, 1], [-1, 8]):
        raw.pins[:] = pins
        assert raw.call(1) == lib.EINVAL
    raw.pins[:] = [-1, 1]
    for sj in (0.0, -1.0, np.inf, np.nan):
        s = raw.s.copy()
        s[2] = sj
        assert raw.call(1, s=s.ctypes.data_as(C.c_void_p)) == lib.EINVAL
        assert raw.call(1, s=s.ctypes.data_as(C.c_void_p), mask=0b011) == lib.OK    # (outside the mask its sum is not looked at)
    for kk in (0, 9, -1):
        assert raw.call(1, k=kk) == lib.EUNSUPPORTED
    assert raw.call(1, dev_in=None, q=None, a_tri=None) == lib.OK                     # (pass 0 consumes no sums)
    free = _Raw(X, H, [-1], np.full((n, k), 0.01))
    assert free.call(1, t=None, slope=None) == lib.OK                                 # (no pinned model: neither t nor slope)


# ---- the fits against the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_full_fit(cml, name):
    X, H, _ = R.case(name)
    got, opt = _full(name), R.optimum(name)
    n, k = X.shape[0], H.shape[0]
    assert got["D"].shape == (n, k) and got["deviance"].shape == got["gap"].shape == got["N"].shape == (n,) and got["deviance_start"] is None
    assert got["converged"].dtype == bool and got["n_pass"].dtype == np.int64 and got["nonfinite"] == 0
    excess = got["deviance"] - opt["deviance"]
    print(f"{name}: passes max {got['n_pass'].max()}, gap max {got['gap'].max():.3g}, dev - dev* max {excess.max():.3g}")
    assert got["converged"].all() and (got["gap"] <= TOL).all()
    assert (excess <= TOL + _slack(got["deviance"])).all() and (excess >= -_slack(got["deviance"])).all()
    assert np.array_equal(got["N"], X.sum(axis=1)) and (got["D"] >= 0).all() and np.isfinite(got["D"]).all()
    live = got["N"] > 0
    assert _close((got["D"] @ H.sum(axis=1))[live], got["N"][live], 1e-13)        # on the ray
    assert got["n_pass"].max() <= R.MAX_PASS // 2


def test_deviance_start_is_the_deviance_at_the_start(cml):
    X, H, D = R.case("A")
    got = cml.ml_channels(X, H, D0=D, max_pass=R.MAX_PASS)
    want = _sums(X, H, np.asarray(D))[0]
    assert _close(got["deviance_start"], want, 1e-11) and got["converged"].all()
    assert (got["deviance_start"] - got["deviance"] >= -TOL - _slack(want)).all()
    assert (got["deviance"] - R.optimum("A")["deviance"] <= TOL + _slack(want)).all()


@pytest.mark.parametrize("name", MULTI)
def test_presence(cml, name):
    X, H, _ = R.case(name)
    got, ref = _presence(name), R.solved(name)
    n, k = X.shape[0], H.shape[0]
    assert got["lr"].shape == got["pvalue"].shape == got["D_ml"].shape == (n, k)
    assert got["converged"].shape == got["gap"].shape == got["n_pass"].shape == (k + 1, n)
    print(f"{name}: nested passes max {got['n_pass'][1:].max()} (reference {ref['n_pass'][1:].max()}), "
          f"|lr - lr_ref| max {np.abs(got['lr'] - ref['lr']).max():.3g}")
    assert got["converged"].all() and (got["gap"] <= TOL).all()
    assert (np.abs(got["lr"] - ref["lr"]) <= 2 * TOL).all()
    assert (got["lr"][got["D_ml"] == 0] == 0).all() and (got["lr"] >= 0).all()
    assert np.array_equal(got["pvalue"], cml.pvalue(got["lr"])) and (got["pvalue"][got["lr"] == 0] == 1).all()
    assert np.array_equal(got["D_ml"], _full(name)["D"]) and np.array_equal(got["deviance_ml"], _full(name)["deviance"])


@pytest.mark.parametrize("name", list(R.CASES))
def test_interval_ends(cml, name):
    """Every end against the long runs of the numpy rule: |phi*(end)| <= lr_tol + tol, phi* = g* - dev* - threshold with the pinned
    deviance g* at tol = 1e-8 and the optimum dev* at 1e-10 (the device's two deviances are each within tol above those, and its own
    phi is within lr_tol of 0)."""
    X, H, _ = R.case(name)
    got, opt = _intervals(name), R.optimum(name)
    n, k = X.shape[0], H.shape[0]
    q = got["threshold"]
    assert got["lower"].shape == got["upper"].shape == (n, k) and got["converged"].shape == got["n_eval"].shape == got["n_pass"].shape == (k, 2, n)
    print(f"{name}: evaluations max {got['n_eval'].max()}, passes per end max {got['n_pass'].max()}")
    assert got["converged"].all() and got["n_eval"].max() <= R.MAX_EVAL // 2
    assert (got["lower"] <= got["D_ml"]).all() and (got["D_ml"] <= got["upper"]).all() and (got["lower"] >= 0).all()
    assert np.array_equal(got["D_ml"], _full(name)["D"])
    # lr at t = 0, to within tol on either side: the reference's nested fits, shared with test_presence (one component: the long run)
    at_zero_all = R.solved(name)["lr"] if k > 1 else (R.profile(X, H, 0, np.zeros(n), opt["D"]) - opt["deviance"])[:, None]
    for j in range(k):
        at_zero = at_zero_all[:, j]
        for side, ends in ((0, got["lower"][:, j]), (1, got["upper"][:, j])):
            phi = R.profile(X, H, j, ends, opt["D"]) - opt["deviance"] - q
            inner = (ends == 0) if side == 0 else np.zeros(n, dtype=bool)
            worst = np.abs(phi[~inner]).max() if (~inner).any() else 0.0
            print(f"  component {j} side {side}: |phi*| max {worst:.3g} over {(~inner).sum()} ends")
            assert (np.abs(phi[~inner]) <= LR_TOL + TOL + _slack(opt["deviance"])[~inner]).all()
            assert (phi[inner] <= TOL + _slack(opt["deviance"])[inner]).all()         # an end AT 0: the profile there is inside the level
        # lower is exactly 0 where lr <= threshold (beyond what the two certificates leave open), and positive where it is above
        assert (got["lower"][:, j][at_zero <= q - 3 * TOL] == 0).all() and (got["lower"][:, j][at_zero >= q + 3 * TOL] > 0).all()
        assert (got["lower"][:, j][got["D_ml"][:, j] == 0] == 0).all()


def test_interval_components_and_level(cml):
    X, H, _ = R.case("A")
    got = cml.intervals(X, H, level=0.68, components=[2], max_pass=R.MAX_PASS)
    full = _intervals("A")
    assert np.isnan(got["lower"][:, :2]).all() and np.isnan(got["upper"][:, :2]).all() and got["converged"][2].all()
    assert not got["n_eval"][:2].any() and got["level"] == 0.68 and got["threshold"] == pytest.approx(R.pn.threshold(0.68))
    assert (got["upper"][:, 2] <= full["upper"][:, 2]).all() and (got["lower"][:, 2] >= full["lower"][:, 2]).all()   # a narrower level


def test_pinned_slope(cml):
    """The slope recomputed in numpy from the returned point (the pinned tests' bound), and against central differences of the numpy
    profile.  For the latter both sides are solved tightly (the device at tol = 1e-9, the profile at 1e-10) at t one standard
    deviation above the optimum, where the profile is smooth, with the step dt = 1e-4 t.  With y >= t h_pin the curvature of the
    profile is at most 2 N / t^2 and its third derivative of the order of N / t^3, so the difference quotient is off by about
    1e-8 N / t; the two profile values carry 1e-10 each, 1e-6 / t in the quotient; and a point within tol of the pinned optimum has a
    gradient within sqrt(2 L tol), L <= 2 N / t^2 the curvature: 6.4e-5 sqrt(N) / t.  Bound: (1e-5 + 1e-4 sqrt(N) + 1e-7 N) / t."""
    X, H, _ = R.case("A")
    n, pin = X.shape[0], 2
    opt = R.optimum("A")
    s, N = H.sum(axis=1), opt["N"]
    t = opt["D"][:, pin] + np.sqrt(N + 1.0) / s[pin]
    got = cml.ml_channels_pinned(X, H, pin, t, D0=opt["D"], tol=1e-9, max_pass=R.MAX_PASS)
    assert got["converged"].all() and np.array_equal(got["D"][:, pin], t)
    dev, q, _ = _sums(X, H, got["D"])
    slope = 2.0 * (s[pin] - q[:, pin])
    assert (np.abs(got["slope"] - slope) <= 1e-9 * (1.0 + 4.0 * s[pin] + np.abs(slope))).all()
    assert (np.abs(got["deviance"] - dev) <= 1e-9 * np.maximum(1.0, np.abs(dev))).all()
    dt = 1e-4 * t
    fd = (R.profile(X, H, pin, t + dt, got["D"], tol=1e-10) - R.profile(X, H, pin, t - dt, got["D"], tol=1e-10)) / (2.0 * dt)
    err = np.abs(got["slope"] - fd)
    bound = (1e-5 + 1e-4 * np.sqrt(N) + 1e-7 * N) / t
    print(f"|slope - central difference| / bound max {(err / bound).max():.3g}")
    assert (err <= bound).all()


# ---- what the lockstep promises bit for bit -----------------------------------------------------------------------------------------------------
KEYS = ("D_ml", "deviance_ml", "lr", "converged", "gap", "n_pass")


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[key], b[key], equal_nan=True) for key in keys)


def test_bits_across_layouts_dtypes_and_padded_rows(cml):
    import torch
    X, H, _ = R.case("A")
    base = _presence("A")
    assert _same(base, cml.presence(np.ascontiguousarray(X.T), H, layout="pm", max_pass=R.MAX_PASS))
    for dt in (np.uint16, np.float32, np.float64, np.int64):     # (int64 narrows to uint8 on the host)
        assert _same(base, cml.presence(X.astype(dt), H, max_pass=R.MAX_PASS)), dt
    padded = torch.zeros((X.shape[0], X.shape[1] + 7), dtype=torch.uint8, device="cuda")
    padded[:, :X.shape[1]] = torch.from_numpy(np.array(X)).cuda()
    padded[:, X.shape[1]:] = 200
    view = padded[:, :X.shape[1]]
    assert view.stride(0) == X.shape[1] + 7
    assert _same(base, cml.presence(view, H, max_pass=R.MAX_PASS))
    assert _same(base, cml.presence(X, H, max_pass=R.MAX_PASS))   # and from call to call


def test_bits_do_not_depend_on_chunk(cml):
    X, H, _ = R.case("A")
    one = cml.intervals(X, H, chunk=1, max_pass=R.MAX_PASS)
    four = _intervals("A")
    assert _same(one, four, ("D_ml", "deviance_ml", "lower", "upper", "converged", "n_eval", "n_pass"))
    assert _same(cml.presence(X, H, chunk=1, max_pass=R.MAX_PASS), _presence("A"))
    assert _same(cml.presence(X, H, chunk=7, max_pass=R.MAX_PASS), _presence("A"))


def test_a_model_alone_and_inside_a_batch(cml):
    """Three pinned models and a free one in one lockstep against each of them alone, and with the others retired from the start in
    two different patterns: the same bits, and a retired model's rows are never written."""
    import torch
    X, H, _ = R.case("A")
    n, k = X.shape[0], H.shape[0]
    sv = cml._Solver(X, H, TOL, R.MAX_PASS, 4, R.LOG_SHIFT, "cm", None, "test")
    sv.upload()
    pins = [0, -1, 2, 1]
    t = torch.from_numpy(np.stack([np.full(n, 0.0), np.zeros(n), np.full(n, 0.02), np.linspace(0.0, 0.05, n)])).cuda()
    start = torch.from_numpy(np.ascontiguousarray(_full("A")["D"])).cuda()
    keys = ("D", "deviance", "gap", "slope", "n_pass", "done")

    def run(models, retired=()):
        d = start[None].repeat(len(models), 1, 1).contiguous()
        done = torch.zeros((len(models), n), dtype=torch.uint8, device="cuda")
        for b in retired:
            done[b] = 1
            d[b] = -3.0
        r = sv.fit(d, [pins[b] for b in models], (1 << k) - 1, t=t[models].contiguous(), done=done)
        return {key: r[key].cpu().numpy().copy() for key in keys}, d.cpu().numpy()

    batch, _ = run([0, 1, 2, 3])
    assert (batch["done"] == 1).all()
    for b in range(4):
        alone, _ = run([b])
        for key in keys:
            if key == "slope" and pins[b] < 0:
                continue
            assert np.array_equal(alone[key][0], batch[key][b]), (b, key)
    for retired in ((0, 2), (1, 3), (3, 2, 0)):
        got, d = run([0, 1, 2, 3], retired)
        for b in range(4):
            if b in retired:
                assert (d[b] == -3.0).all()                      # its d rows were never written
                continue
            for key in keys:
                if key == "slope" and pins[b] < 0:
                    continue
                assert np.array_equal(got[key][b], batch[key][b]), (retired, b, key)


# ---- the estimator ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _estimator():
    from espm_amd.estimators import SmoothNMF
    X, H, D = R.case("A")
    # G=None: W_ is the spectra themselves; started at the truth, so that component j stays the one whose holes were planted
    est = SmoothNMF(n_components=3, shape_2d=(20, 30), max_iter=60, tol=0.0, verbose=0, simplex_W=False)
    quiet(est.fit_transform, np.asarray(X, dtype=np.float32), W=np.maximum(np.array(D), 1e-6), H=np.maximum(np.array(H), 1e-6))
    return est


def test_estimator_spectrum_presence(cml):
    from espm_amd import hyperspy_adapter
    X, H, D = R.case("A")
    est = _estimator()
    n, k = 40, 3
    assert est._identity_G
    windows = [(5, 9), (12, 13), (0, 40)]
    out = est.spectrum_presence(X=X, windows=windows)
    assert est.D_ml_.shape == est.D_presence_lr_.shape == est.D_presence_pvalue_.shape == (n, k)
    assert est.D_deviance_ml_.shape == est.D_excess_deviance_.shape == (n,) and est.D_ml_converged_.shape == (k + 1, n)
    assert est.line_presence_lr_.shape == est.line_presence_pvalue_.shape == (3, k)
    assert est.D_ml_converged_.all()
    dev = est.D_deviance_ml_ + est.D_excess_deviance_
    print(f"excess deviance: min {est.D_excess_deviance_.min():.3g}, max {est.D_excess_deviance_.max():.3g}")
    assert (est.D_excess_deviance_ >= -1e-9 * np.maximum(1.0, dev)).all()
    assert np.array_equal(out["line_lr"], est.line_presence_lr_) and np.array_equal(out["lr"], est.D_presence_lr_)
    assert _close(est.line_presence_lr_[0], est.D_presence_lr_[5:9].sum(axis=0), 1e-14)
    assert np.array_equal(est.line_presence_pvalue_[1], est.D_presence_pvalue_[12])    # one channel: the channel's own p-value
    # the planted holes have the smallest lr of their column
    live = np.asarray(X).sum(axis=1) > 0
    for lo, hi, j in R.CASES["A"]["holes"]:
        rest = np.setdiff1d(np.flatnonzero(live), np.arange(lo, hi))
        print(f"holes of column {j}: lr max {est.D_presence_lr_[lo:hi, j].max():.3g}, the rest min {est.D_presence_lr_[rest, j].min():.3g}")
        assert est.D_presence_lr_[lo:hi, j].max() <= est.D_presence_lr_[rest, j].min()
    bands = hyperspy_adapter.spectrum_bands(est)
    assert bands["lr"].shape == (k, n) and np.array_equal(bands["D_ml"], est.D_ml_.T)
    # from the fit's own image the same tables come to rounding of the un-scaled X_ (not bit for bit: X_ is float32)
    again = est.spectrum_presence()
    assert again["converged"].all() and np.abs(again["lr"] - out["lr"]).max() <= 2 * TOL + 1e-6 * np.abs(out["lr"]).max()
    with pytest.raises(NotImplementedError, match="element_presence: needs a dictionary or physics model G"):
        est.element_presence(X=X)


def test_estimator_spectrum_intervals(cml):
    from espm_amd import hyperspy_adapter
    X, H, D = R.case("A")
    est = _estimator()
    n, k = 40, 3
    out = est.spectrum_intervals(X=X, components=[0, 2])
    assert est.D_lower_.shape == est.D_upper_.shape == est.D_ml_.shape == (n, k) and est.D_interval_level_ == 0.95
    assert est.D_interval_converged_.shape == est.D_interval_n_eval_.shape == (k, 2, n)
    assert est.D_interval_converged_[[0, 2]].all() and np.isnan(est.D_upper_[:, 1]).all() and not np.isnan(est.D_upper_[:, [0, 2]]).any()
    assert (est.D_lower_[:, [0, 2]] <= est.D_ml_[:, [0, 2]]).all() and (est.D_ml_[:, [0, 2]] <= est.D_upper_[:, [0, 2]]).all()
    assert np.array_equal(out["upper"], est.D_upper_, equal_nan=True)
    bands = hyperspy_adapter.spectrum_bands(est)
    assert bands["upper"].shape == (k, n) and bands["level"] == 0.95
