"""Weighted marginals without a device: the weight builders against hand-written cases and their restated rules, the numpy reference
(tests/marginals_reference.py) in the kernel's order and in extended precision against its own bounds, the planted line of the line-map
test, the binding, the argument checks of the entry point that come before any launch, the wide builds' stubs, and what the module, the
estimator and the adapter refuse before anything is uploaded."""
import ctypes as C

import numpy as np
import pytest

from abi_header import CTYPE, _declared
import marginals_reference as mr

N, SHAPE = 96, (40, 33)
P = SHAPE[0] * SHAPE[1]
SHAPES = [(96, (40, 33), 20, 500), (300, (7, 10), 20, 33), (16, (50, 50), 5, 500)]   # (n, grid, the zero row of D, the zero column of H)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def marginals():
    from espm_amd import marginals
    return marginals


# ---- the weight builders --------------------------------------------------------------------------------------------------------------------
def test_window_weights(marginals):
    U = marginals.window_weights(8, [(0, 3), (2, 5), (7, 8), (0, 8)])   # overlap, the first and the last channel, everything
    assert U.dtype == np.float64 and np.array_equal(U, [[1, 1, 1, 0, 0, 0, 0, 0], [0, 0, 1, 1, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1], [1] * 8])
    assert np.array_equal(U, mr.window_weights(8, [(0, 3), (2, 5), (7, 8), (0, 8)]))
    assert np.array_equal(marginals.window_weights(5, [(np.int64(1), np.int32(2))]), [[0, 1, 0, 0, 0]])
    for bad in ([(3, 3)], [(4, 2)], [(-1, 2)], [(0, 9)], [(0.5, 2)], [3], []):
        with pytest.raises(ValueError):
            marginals.window_weights(8, bad)
    with pytest.raises(ValueError):
        marginals.window_weights(0, [(0, 1)])


def test_line_weights(marginals):
    assert np.array_equal(marginals.line_weights(6, (2, 4)), [0, 0, 1, 1, 0, 0])
    # symmetric side windows: c_I = 4.5, c_L = 1.5, c_R = 7.5, s = 1 / 2; 2 channels of background, half from either side
    u = marginals.line_weights(10, (4, 6), ((1, 3), (7, 9)))
    assert u.dtype == np.float64 and np.array_equal(u, [0, -0.5, -0.5, 0, 1, 1, 0, -0.5, -0.5, 0])
    # a line at the image's first and last channel, windows of different widths: c_I = 0, c_L = 2.5, c_R = 8, s = -2.5 / 5.5
    u = marginals.line_weights(10, (0, 1), ((1, 5), (7, 10)))
    s = (0 - 2.5) / (8 - 2.5)
    want = np.zeros(10)
    want[0] = 1
    want[1:5] -= (1 - s) / 4
    want[7:10] -= s / 3
    assert s < 0 and np.array_equal(u, want) and np.array_equal(u, mr.line_weights(10, (0, 1), ((1, 5), (7, 10))))
    u = marginals.line_weights(10, (9, 10), ((0, 2), (4, 8)))   # both windows below the line: s = (9 - 0.5) / (5.5 - 0.5) = 1.7
    assert np.allclose(u, [0.35, 0.35, 0, 0, -0.425, -0.425, -0.425, -0.425, 0, 1], rtol=0, atol=1e-15)
    # the rule's two invariants: a flat spectrum and a linear one have net 0 (the interpolation is exact for them)
    for args in (((4, 6), ((1, 3), (7, 9))), ((0, 1), ((1, 5), (7, 10))), ((9, 10), ((0, 2), (4, 8))), ((3, 7), ((2, 5), (4, 9)))):
        u = marginals.line_weights(10, *args)
        assert abs(u.sum()) < 1e-14 and abs((u * np.arange(10)).sum()) < 1e-13
        assert np.allclose(u, mr.line_weights(10, *args), rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="centred"):
        marginals.line_weights(10, (4, 6), ((1, 4), (2, 3)))   # c_L == c_R == 2
    for bad in (((4, 4), None), ((4, 6), ((1, 3),)), ((4, 6), ((1, 3), (7, 11))), ((4, 6), ((3, 1), (7, 9))), ((4, 6), 5)):
        with pytest.raises(ValueError):
            marginals.line_weights(10, *bad)


def test_label_weights(marginals):
    lab = np.array([[0, 2, -1], [2, 2, 0]])
    W = marginals.label_weights(lab)   # region 1 is empty, pixel 2 belongs to none
    assert W.dtype == np.float64 and np.array_equal(W, [[1, 0, 0, 0, 0, 1], [0] * 6, [0, 1, 0, 1, 1, 0]])
    assert np.array_equal(W, mr.label_weights(lab))
    assert marginals.label_weights(lab, n_regions=4).shape == (4, 6) and not marginals.label_weights(lab, n_regions=4)[3].any()
    assert np.array_equal(marginals.label_weights(np.array([1, 1], dtype=np.uint8)), [[0, 0], [1, 1]])
    for bad, kw in ((lab, dict(n_regions=2)), (lab.astype(float), {}), (np.array([-1, -1]), {}), (np.zeros(0, int), {})):
        with pytest.raises(ValueError):
            marginals.label_weights(bad, **kw)


# ---- the reference against its own bounds ------------------------------------------------------------------------------------------------------
def _mixed_weights(m, lo, hi):
    """A window, a signed line vector and an all-zero vector over an axis of m."""
    w = hi - lo
    return np.stack([mr.window_weights(m, [(lo, hi)])[0], mr.line_weights(m, (lo, hi), ((lo - w, lo - 2), (hi + 1, hi + w + 3))), np.zeros(m)])


@pytest.mark.parametrize("n,shape,channel,pixel", SHAPES)
@pytest.mark.parametrize("side", ["pixels", "channels"])
def test_reference_in_the_kernels_order_keeps_its_bounds(side, n, shape, channel, pixel):
    """The fp64 reference against the rule evaluated in the kernel's order in extended precision (the exact value, for this purpose) and
    in fp64 (the device's arithmetic less its fused multiply-adds): both within the derived bounds, with the room printed."""
    p = shape[0] * shape[1]
    X = mr.image(n, shape, np.uint16)
    D, H = mr.planted_model(n, p, 3, channel, pixel)
    m = n if side == "pixels" else p
    W = _mixed_weights(m, m // 3, m // 3 + max(4, m // 12))
    ref = mr.sums(X, W, D, H, side)
    assert ref["counts"].shape == (3, p if side == "pixels" else n) and not ref["counts_exact"]   # (the line vector is not integer)
    assert (ref["deviance_bound"][:2] > 0).all() and not ref["deviance_bound"][2].any()
    for ft in (np.longdouble, np.float64):
        got = mr.in_kernel_order(X, W, D, H, side, ft=ft)
        for name, v in zip(("counts", "model", "deviance"), got):
            err = np.abs(v.astype(np.longdouble) - ref[name])
            b = ref[name + "_bound"]
            room = float((err / np.where(b > 0, b, 1)).max())
            print(f"{n} x {p}, {side}, {np.dtype(ft).name}: {name} worst error / bound {room:.3g}")
            assert (err <= b).all(), (name, room)
    # integer weights: the counts are the int64 sums, bit for bit, in any order
    ref = mr.sums(X, W[[0, 2]], D, H, side)
    got = mr.in_kernel_order(X, W[[0, 2]], side=side, ft=np.float64)[0]
    assert ref["counts_exact"] and not ref["counts_bound"].any() and np.array_equal(got, ref["counts"])
    Xi = X.astype(np.int64)
    assert np.array_equal(ref["counts"][0], (Xi[m // 3:m // 3 + max(4, m // 12)].sum(axis=0) if side == "pixels"
                                             else Xi[:, m // 3:m // 3 + max(4, m // 12)].sum(axis=1)))
    # where the model is zero the floor stands: Y = log_shift under whatever counts are there
    x, Y, t, mag = mr.pieces(X, D, H)
    assert (Y[channel] == mr.LOG_SHIFT).all() and (Y[:, pixel] == mr.LOG_SHIFT).all() and X[channel].any() and np.isfinite(t).all()


def test_the_planted_line_is_recovered_by_the_reference():
    """The condition of the GPU test, checked here first: at the committed seed the numpy line map misses the planted counts by more
    than 5 net_std on at most LINE_SHARE of the pixels (none, in fact)."""
    X, planted = mr.planted_line()
    u = mr.line_weights(N, *mr.LINE)
    x = X.astype(np.float64)
    net, std = u @ x, np.sqrt((u * u) @ x)
    share = mr.line_misses(net, std, planted)
    z = (net - planted) / std
    print(f"planted line: {share:.4f} of the pixels beyond 5 net_std; z mean {z.mean():+.3f}, std {z.std():.3f}, worst {np.abs(z).max():.2f}")
    assert share <= mr.LINE_SHARE and abs(z.mean()) < 0.2 and 0.8 < z.std() < 1.2
    raw = x[40:48].sum(axis=0)
    assert (raw - planted).mean() > 10   # (without the correction the window holds 16 background counts too)


# ---- the binding ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["espm_weighted_marginals", "espm_weighted_marginals_scratch"])
def test_symbols_are_bound_with_the_headers_signatures(lib, name):
    res, args = lib.SYMBOLS[name]
    cres, cargs = _declared(name)
    assert res is CTYPE[cres]
    assert list(args) == [CTYPE[a] for a in cargs]
    for handle in (lib.lib, lib.variant(12).lib, lib.variant(20).lib):
        assert hasattr(handle, name)


def test_header_carries_the_sizes(lib, marginals):
    from espm_amd import _abi
    d = _abi.parse_defines(_abi.header_text())
    assert d["ESPM_MARG_MAX_G"] == lib.MARG_MAX_G == marginals.MAX_G == mr.MAX_G == 8
    assert d["ESPM_MARG_MAX_K"] == lib.MARG_MAX_K == marginals.MAX_K == mr.MAX_K == lib.DIAG_MAX_K
    assert d["ESPM_MARG_PCHUNK"] == lib.MARG_PCHUNK == mr.PCHUNK == lib.CDIAG_PCHUNK and lib.MARG_BLOCK == 256
    assert (lib.MARG_PIXELS, lib.MARG_CHANNELS) == (0, 1)


U8, F64, CM, PM, PIX, CHAN = 0, 3, 0, 1, 0, 1


def _vp(v):
    return None if v is None else C.c_void_p(v)   # (never dereferenced: every call below is refused on the host)


def _call(f, x=8, dtype=U8, layout=CM, ld=80, n=8, p=80, side=PIX, wgt=8, g=3, d=8, h=8, k=3, log_shift=1e-14, xs=8, ys=8, dev=8, scratch=8,
          scratch_bytes=1 << 20):
    return f(_vp(x), dtype, layout, ld, n, p, side, _vp(wgt), g, _vp(d), _vp(h), k, log_shift, _vp(xs), _vp(ys), _vp(dev), _vp(scratch),
             scratch_bytes, None)


def test_argument_errors_need_no_device(lib):
    f, err = lib.lib.espm_weighted_marginals, lib.lib.espm_mu_last_error
    for side in (PIX, CHAN):
        for name in ("x", "wgt", "xs", "d", "h", "ys", "dev"):
            assert _call(f, side=side, **{name: None}) == lib.EINVAL, name
    assert _call(f, side=CHAN, scratch=None) == lib.EINVAL and b"scratch" in err()
    assert _call(f, side=2) == lib.EINVAL and b"side 2" in err()
    assert _call(f, side=-1) == lib.EINVAL and b"side -1" in err()
    assert _call(f, layout=2) == lib.EINVAL and b"x_layout 2" in err()
    assert _call(f, dtype=4) == lib.EINVAL and b"x_dtype 4" in err()
    assert _call(f, dtype=-1) == lib.EINVAL
    assert _call(f, g=0) == lib.EINVAL and b"g=0" in err()
    assert _call(f, g=9) == lib.EINVAL and b"g=9" in err()
    assert _call(f, k=-1) == lib.EINVAL and b"k=-1" in err()
    assert _call(f, k=9) == lib.EINVAL and b"k=9" in err()
    assert _call(f, n=0) == lib.EINVAL and b"n=0" in err()
    assert _call(f, p=0) == lib.EINVAL and b"p=0" in err()
    assert _call(f, ld=79) == lib.EINVAL and b"ld=79" in err()
    assert _call(f, layout=PM, ld=7) == lib.EINVAL and b"ld=7" in err()      # pixel-major: rows of n
    assert _call(f, log_shift=0.0) == lib.EINVAL and b"log_shift=0" in err()
    assert _call(f, log_shift=-1.0) == lib.EINVAL and _call(f, log_shift=float("nan")) == lib.EINVAL
    # k = 0: no model, no model sums - and then log_shift is not looked at
    for name in ("d", "h", "ys", "dev"):
        args = dict(d=None, h=None, ys=None, dev=None, k=0)
        args[name] = 8
        assert _call(f, **args) == lib.EINVAL and b"k=0" in err(), name
    assert _call(f, k=0, d=None, h=None, ys=None, dev=None, log_shift=0.0, x=None) == lib.EINVAL and b"bad arguments" in err()
    # the scratch: chunks x 3 x g x n doubles on the channel side, nothing on the pixel side
    q = lib.lib.espm_weighted_marginals_scratch
    assert q(CHAN, 8, 80, 3) == 1 * 3 * 3 * 8 * 8 and q(CHAN, 16, 2500, 8) == 2 * 3 * 8 * 16 * 8 and q(CHAN, 2048, 512 * 512, 8) == 128 * 3 * 8 * 2048 * 8
    assert q(PIX, 8, 80, 3) == q(2, 8, 80, 3) == q(CHAN, 0, 80, 3) == q(CHAN, 8, 0, 3) == q(CHAN, 8, 80, 0) == q(CHAN, 8, 80, 9) == 0
    assert _call(f, side=CHAN, scratch_bytes=q(CHAN, 8, 80, 3) - 1) == lib.EINVAL and b"575 bytes, 576 needed" in err()
    assert _call(f, side=CHAN, n=65535 * 256 + 1, p=1, ld=1) == lib.EINVAL and b"n=16776961" in err()


def test_the_wide_builds_export_stubs(lib):
    for k in (12, 20):
        v = lib.variant(k)
        rc = v.lib.espm_weighted_marginals(None, 0, 0, 8, 8, 8, 0, None, 1, None, None, 0, 1e-14, None, None, None, None, 0, None)
        assert rc == lib.EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            v.check(rc)
        assert v.lib.espm_weighted_marginals_scratch(1, 96, 1320, 3) == 0 and lib.lib.espm_weighted_marginals_scratch(1, 96, 1320, 3) > 0


# ---- the Python module, the estimator and the adapter, before the device ---------------------------------------------------------------------
def test_module_raises_before_upload(lib, marginals, monkeypatch):
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X = np.zeros((6, 20), np.uint8)
    D, H = np.ones((6, 2)), np.ones((2, 20))
    Wn, Wp = np.ones((2, 6)), np.ones((2, 20))
    for call, W, other in ((marginals.pixel_maps, Wn, Wp), (marginals.channel_spectra, Wp, Wn)):
        with pytest.raises(ValueError, match="layout"):
            call(X, W, layout="rows")
        with pytest.raises(ValueError, match="2-D"):
            call(np.zeros(6, np.uint8), W)
        with pytest.raises(ValueError, match="weights of shape"):
            call(X, other)
        with pytest.raises(ValueError, match="weights of shape"):
            call(X, np.ones((2, 3, 4)))
        with pytest.raises(ValueError, match="weights of shape"):
            call(X, W, layout="pm")   # (pixel-major: the 6 x 20 array is 6 pixels of 20 channels)
        with pytest.raises(ValueError, match="not finite"):
            call(X, np.where(np.arange(W.size).reshape(W.shape) == 3, np.nan, W))
        with pytest.raises(ValueError, match="not finite"):
            call(np.where(np.arange(120).reshape(6, 20) == 7, np.inf, 0.0), W)
        with pytest.raises(ValueError, match="from -1 to 0"):
            call(X.astype(np.int32) - (np.arange(120).reshape(6, 20) == 7), W)
        with pytest.raises(ValueError, match="D and H together"):
            call(X, W, D=D)
        with pytest.raises(ValueError, match="channels"):
            call(X, W, np.ones((5, 2)), H)
        with pytest.raises(ValueError, match="pixels"):
            call(X, W, D, np.ones((2, 19)))
        with pytest.raises(ValueError, match="components"):
            call(X, W, np.ones((6, 2)), np.ones((3, 20)))
        with pytest.raises(ValueError, match="log_shift"):
            call(X, W, D, H, log_shift=0)
        with pytest.raises(NotImplementedError, match="9 components"):
            call(X, W, np.ones((6, 9)), np.ones((9, 20)))
    for lines in ([], [((2, 4),)], [((4, 2), None)], [((2, 4), ((0, 1), (0, 1)))], [((2, 7), None)]):
        with pytest.raises(ValueError):
            marginals.line_maps(X, lines)
    with pytest.raises(ValueError, match="X has 6 channels"):
        marginals.line_maps(X, [((2, 4), None)], np.ones((5, 2)), H)
    with pytest.raises(NotImplementedError, match="33 components"):
        marginals.line_maps(X, [((2, 4), None)], np.ones((6, 33)), np.ones((33, 20)))


def test_no_cpu_fallback(lib, marginals, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X = np.zeros((6, 20), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        marginals.pixel_maps(X, np.ones((1, 6)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        marginals.channel_spectra(X, np.ones((1, 20)), np.ones((6, 2)), np.ones((2, 20)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        marginals.line_maps(X, [((2, 4), None)])


def _fitted(**kw):
    """An estimator with the attributes of a fit (the fit itself needs the device)."""
    from espm_amd.estimators import SmoothNMF
    args = dict(n_components=3, shape_2d=(4, 5), max_iter=5, verbose=0)
    args.update(kw)
    est = SmoothNMF(**args)
    k = args["n_components"]
    est.G_, est.W_, est.H_, est._identity_G = np.eye(6), np.ones((6, k)), np.ones((k, 20)) / k, True
    est.X_ = np.ones((6, 20))
    return est


def test_estimator_refuses_before_any_upload(lib, marginals, monkeypatch):
    from sklearn.exceptions import NotFittedError

    from espm_amd.estimators import SmoothNMF
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X = np.ones((6, 20), np.uint8)
    lines = [((2, 4), ((0, 2), (4, 6)))]
    labels = np.arange(20) % 3
    with pytest.raises(NotFittedError):
        SmoothNMF(n_components=3, verbose=0).line_maps(lines, X)
    with pytest.raises(NotFittedError):
        SmoothNMF(n_components=3, verbose=0).region_spectra(labels, X)
    for call, arg in ((lambda e, x: e.line_maps(lines, x), None), (lambda e, x: e.region_spectra(labels, x), None)):
        with pytest.raises(ValueError, match="X has 5 channels"):
            call(_fitted(), X[:5])
        with pytest.raises(ValueError, match="X has 19 pixels"):
            call(_fitted(), X[:, :19])
        with pytest.raises(ValueError, match="X has 20 channels"):
            call(_fitted(hspy_comp=True), X)
        binned = _fitted()
        binned.bin_ = (2, 2)
        with pytest.raises(ValueError, match="fit_binned"):
            call(binned, None)
    with pytest.raises(ValueError):
        _fitted().line_maps([((2, 9), None)], X)
    with pytest.raises(ValueError, match="label map of 19 pixels"):
        _fitted().region_spectra(labels[:19], X)
    with pytest.raises(ValueError, match="weights of shape"):
        _fitted().region_spectra(np.ones((2, 19)), X)
    with pytest.raises(ValueError, match="weights of shape"):
        _fitted().region_spectra(np.ones(20), X)
    with pytest.raises(NotImplementedError, match="9 components"):
        _fitted(n_components=9).region_spectra(labels, X)
    est = _fitted()
    for name in ("lines_", "line_net_", "region_counts_", "region_pixels_"):
        assert not hasattr(est, name)


def test_adapter_needs_the_analyses_first(lib):
    from espm_amd import hyperspy_adapter as ha
    est = _fitted()
    with pytest.raises(AttributeError, match=r"call est.line_maps\(\) first"):
        ha.line_maps(est)
    with pytest.raises(AttributeError, match=r"call est.region_spectra\(\) first"):
        ha.region_spectra(est)
    est.line_net_, est.line_net_std_, est.line_model_ = (np.arange(40.0).reshape(2, 20) + i for i in range(3))
    est.line_components_ = np.arange(120.0).reshape(2, 3, 20)
    net, std, model, comp = ha.line_maps(est)
    assert net.shape == std.shape == model.shape == (2, 4, 5) and comp.shape == (2, 3, 4, 5)
    assert np.array_equal(net.reshape(2, 20), est.line_net_) and ha.line_maps(est, shape_2d=(2, 10))[3].shape == (2, 3, 2, 10)
    est.region_counts_, est.region_model_, est.region_deviance_ = (np.arange(12.0).reshape(6, 2) + i for i in range(3))
    counts, model, deviance = ha.region_spectra(est)
    assert counts.shape == (2, 6) and np.array_equal(counts, est.region_counts_.T) and np.array_equal(deviance, est.region_deviance_.T)
    sig = ha.SpectrumImage(np.zeros((4, 5, 6), np.uint8))
    with pytest.raises(ValueError, match="labels of shape"):
        sig.region_spectra(np.zeros((5, 4), int))
