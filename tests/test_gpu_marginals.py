"""Weighted marginals on the device against their numpy restatement (tests/marginals_reference.py): both sides, the four dtypes and both
layouts within the derived bounds and bit-equal where that is promised, component and group counts, all-ones weights against the
diagnostics' own sums bit for bit, the workgroup-uniform skip, strided rows, line maps with a planted line, the estimator's methods
and the adapter's shapes.

The image is the splitting tests' 96 channels x 40 x 33 pixels: 1320 pixels are a ragged last wave and workgroup, 96 channels cross a
transposing tile of 64, 32 or 16 rows; the model has an all-zero row of D and all-zero columns of H.  300 channels x 7 x 10 pixels run
a second, ragged staging round of the pixel side (256 + 44), 16 channels x 50 x 50 pixels two chunks of the channel side
(2048 + 452)."""
import functools

import numpy as np
import pytest

import marginals_reference as mr

pytestmark = pytest.mark.gpu

N, SHAPE = 96, (40, 33)
P = SHAPE[0] * SHAPE[1]
GEOMETRY = {96: ((40, 33), 20, 500), 300: ((7, 10), 20, 33), 16: ((50, 50), 5, 500)}   # n: (grid, the zero row of D, the zero column of H)
SIDES = ["pixels", "channels"]


@pytest.fixture(scope="module")
def marginals():
    from espm_amd import marginals
    return marginals


@functools.lru_cache(maxsize=None)
def _image(n, dtype):
    return mr.image(n, GEOMETRY[n][0], np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def _model(n, k):
    shape, channel, pixel = GEOMETRY[n]
    return mr.planted_model(n, shape[0] * shape[1], k, channel, pixel)


def _mixed(m):
    """A window, a signed line vector and an all-zero vector over an axis of m."""
    lo = m // 3
    hi = lo + max(4, m // 12)
    w = hi - lo
    return np.stack([mr.window_weights(m, [(lo, hi)])[0], mr.line_weights(m, (lo, hi), ((lo - w, lo - 2), (hi + 1, hi + w + 3))), np.zeros(m)])


def _dense(g, m, seed=1):
    """g weight vectors without a zero: signed, a few bits each (so that products with counts are cheap to reason about)."""
    rng = np.random.default_rng(seed)
    return rng.integers(1, 9, size=(g, m)) / 4.0 * np.where(rng.random((g, m)) < 0.3, -1.0, 1.0)


def _lay(X, layout):
    return X if layout == "cm" else np.ascontiguousarray(X.T)


def _code(dtype):
    from espm_amd import _lib
    return {"uint8": _lib.DIAG_X_U8, "uint16": _lib.DIAG_X_U16, "float32": _lib.DIAG_X_F32, "float64": _lib.DIAG_X_F64}[np.dtype(dtype).name]


def _raw(X, W, D=None, H=None, side="pixels", layout="cm", pad=0, short=0):
    """espm_weighted_marginals itself on X (n, p) handed over in ``layout``: (counts, model, deviance), each (g, lanes), the last two None
    without a model.  With ``pad`` the rows of X are that much longer than they say, the padding full of counts that must not be read,
    and the outputs have a spare row whose fill must stay.  ``short``: bytes the scratch is declared too small by (returns the status)."""
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    n, p = X.shape
    k = 0 if D is None else D.shape[1]
    g = W.shape[0]
    Xin = _lay(X, layout)
    rows, cols = Xin.shape
    wide = np.full((rows, cols + pad), 201, dtype=X.dtype)
    wide[:, :cols] = Xin
    Xd = torch.from_numpy(wide).to("cuda")
    Wd = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float64)).to("cuda")
    Dd, Hd = (torch.from_numpy(np.ascontiguousarray(D)).to("cuda"), torch.from_numpy(np.ascontiguousarray(H)).to("cuda")) if k else (None, None)
    code = _lib.MARG_PIXELS if side == "pixels" else _lib.MARG_CHANNELS
    m = p if side == "pixels" else n
    outs = [torch.full((g + 1, m), -77.0, dtype=torch.float64, device="cuda") for _ in range(3 if k else 1)] + [None, None]
    need = int(_lib.lib.espm_weighted_marginals_scratch(code, n, p, g))
    assert need == (0 if side == "pixels" else -(-p // mr.PCHUNK) * 3 * g * n * 8)
    scratch = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = _lib.lib.espm_weighted_marginals(_ptr(Xd), _code(X.dtype), _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM, cols + pad, n, p, code,
                                          _ptr(Wd), g, _ptr(Dd), _ptr(Hd), k, mr.LOG_SHIFT, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                                          _ptr(scratch), need - short, _stream())
    if short:
        return rc
    _lib.check(rc)
    got = [o.cpu().numpy() for o in outs[:3 if k else 1]]
    assert all((o[g] == -77.0).all() for o in got), "the spare row of an output was written"
    assert (scratch[need:].cpu().numpy() == 0x5A).all(), "the scratch was written past its size"
    got = [o[:g] for o in got]
    return got[0], (got[1] if k else None), (got[2] if k else None)


def _within(got, ref, what):
    for name, v in zip(("counts", "model", "deviance"), got):
        if v is None:
            assert ref[name] is None
            continue
        err = np.abs(v - ref[name])
        b = ref[name + "_bound"]
        worst = float((err / np.where(b > 0, b, 1.0)).max())
        print(f"{what}: {name} worst error / bound {worst:.3g}")
        assert (err <= b).all(), (what, name, worst)
    if ref["counts_exact"]:
        assert np.array_equal(got[0], ref["counts"]), what


def _same(a, b):
    return all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(a, b))


# ---- both sides, the four dtypes, both layouts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32", "float64"])
def test_sums_are_within_the_derived_bounds(dtype, side):
    X = _image(N, dtype)
    D, H = _model(N, 3)
    W = _mixed(N if side == "pixels" else P)
    ref = mr.sums(X, W, D, H, side)
    cm = _raw(X, W, D, H, side, "cm")
    _within(cm, ref, f"{dtype}, {side}")
    assert _same(cm, _raw(X, W, D, H, side, "pm")), "the two layouts differ"
    assert _same(cm, _raw(X, W, D, H, side, "cm")), "two calls differ"
    assert all(not v[2].any() for v in cm)   # the all-zero vector
    # the window alone has integer weights: its counts are the integer sums, bit for bit (in every dtype: the counts are integers)
    exact = mr.sums(X.astype(np.int64), W[[0, 2]], side=side)
    assert exact["counts_exact"] and np.array_equal(cm[0][[0, 2]], exact["counts"])
    # where the model is zero, Y is the floor: the planted pixel's modelled window is (hi - lo) log_shift (within the bound, above)
    if side == "pixels":
        assert 0 < cm[1][0, 500] < 1e-12 < cm[1][0, 499]


# ---- component and group counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("g", [1, 8])
@pytest.mark.parametrize("k", [0, 1, 5, 8])
def test_component_and_group_counts(k, g, side):
    X = _image(N, "uint16")
    D, H = _model(N, k) if k else (None, None)
    W = _dense(g, N if side == "pixels" else P)
    W[0] = _mixed(W.shape[1])[1]
    ref = mr.sums(X, W, D, H, side)
    cm = _raw(X, W, D, H, side, "cm")
    _within(cm, ref, f"k = {k}, g = {g}, {side}")
    assert _same(cm, _raw(X, W, D, H, side, "pm"))


def test_more_groups_than_a_launch_and_more_components_than_the_kernels(marginals):
    X = _image(N, "uint8")
    D, H = _model(N, 3)
    for call, side, m in ((marginals.pixel_maps, "pixels", N), (marginals.channel_spectra, "channels", P)):
        W = _dense(9, m)
        ref = mr.sums(X, W, D, H, side)
        out = call(X, W, D, H)
        got = [out[name] if side == "pixels" else out[name].T for name in ("counts", "model", "deviance")]
        assert got[0].shape == (9, P if side == "pixels" else N)
        _within(got, ref, f"g = 9, {side}")
        one = _raw(X, W[8:], D, H, side)   # the second batch is the launch of its one vector
        assert all(np.array_equal(v[8:], w) for v, w in zip(got, one))
        pm = call(_lay(X, "pm"), W, D, H, layout="pm")
        assert all(np.array_equal(out[name], pm[name]) for name in out)
        raw = call(X, W[:2])
        assert raw["model"] is None and raw["deviance"] is None and np.array_equal(raw["counts"], out["counts"][:2] if side == "pixels" else out["counts"][:, :2])
        # other integer dtypes are narrowed after their range check, a device tensor is taken where it is
        import torch
        assert np.array_equal(call(X.astype(np.int64), W[:2])["counts"], raw["counts"])
        assert np.array_equal(call(torch.from_numpy(X.astype(np.int32)).to("cuda"), W[:2])["counts"], raw["counts"])
        with pytest.raises(NotImplementedError, match="9 components"):
            call(X, W, *_model(N, 9))


# ---- all weights 1: the diagnostics' own sums, bit for bit ---------------------------------------------------------------------------------
def _diagnostics(X, D, H, layout):
    """(dev (p,)) of espm_pixel_diagnostics and (dev, xsum, ysum (n,)) of espm_channel_diagnostics on the same inputs."""
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    n, p = X.shape
    k = D.shape[1]
    Xd = torch.from_numpy(_lay(X, layout)).to("cuda")
    Dd, Hd = torch.from_numpy(np.ascontiguousarray(D)).to("cuda"), torch.from_numpy(np.ascontiguousarray(H)).to("cuda")
    lay = _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM
    dev, hstd = torch.empty(p, dtype=torch.float64, device="cuda"), torch.empty((k, p), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib.espm_pixel_diagnostics(_ptr(Xd), _code(X.dtype), lay, int(Xd.stride(0)), n, p, _ptr(Dd), _ptr(Hd), k, mr.LOG_SHIFT, 0,
                                               _ptr(dev), _ptr(hstd), None, _stream()))
    cdev, xsum, ysum = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(3))
    tri = torch.empty((n, k * (k + 1) // 2), dtype=torch.float64, device="cuda")
    need = int(_lib.lib.espm_channel_diagnostics_scratch(n, p, k))
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.espm_channel_diagnostics(_ptr(Xd), _code(X.dtype), lay, int(Xd.stride(0)), n, p, _ptr(Dd), _ptr(Hd), k, mr.LOG_SHIFT,
                                                 _ptr(cdev), _ptr(xsum), _ptr(ysum), _ptr(tri), _ptr(scratch), need, _stream()))
    return dev.cpu().numpy(), cdev.cpu().numpy(), xsum.cpu().numpy(), ysum.cpu().numpy()


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("n", [96, 16])
def test_all_ones_weights_are_the_diagnostics_sums(n, k, layout):
    X = _image(n, "uint16")
    p = X.shape[1]
    D, H = _model(n, k)
    dev, cdev, xsum, ysum = _diagnostics(X, D, H, layout)
    pix = _raw(X, np.ones((2, n)), D, H, "pixels", layout)
    assert np.array_equal(pix[2][0], dev) and np.array_equal(pix[2][1], dev)
    chan = _raw(X, np.ones((1, p)), D, H, "channels", layout)
    assert np.array_equal(chan[0][0], xsum) and np.array_equal(chan[1][0], ysum) and np.array_equal(chan[2][0], cdev)
    assert dev.sum() > 0 and np.array_equal(xsum, X.astype(np.int64).sum(axis=1))


# ---- the workgroup-uniform skip --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("side,n", [("pixels", 300), ("pixels", 96), ("channels", 96), ("channels", 16)])
def test_skipped_indices_change_no_bit(side, n, k, layout):
    """Two narrow windows leave most walk indices, whole tiles and whole staging rounds without a weight: the skip is on.  The same two
    windows among two dense vectors of other groups: no index is skipped.  The same bits, and the reference's values."""
    X = _image(n, "uint16")
    p = X.shape[1]
    D, H = _model(n, k) if k else (None, None)
    m = n if side == "pixels" else p
    narrow = np.zeros((2, m))
    narrow[0, m // 2:m // 2 + 3] = 1.0
    narrow[1, [1, m // 2 + 1]] = [-0.5, 2.0]
    ref = mr.sums(X, narrow, D, H, side)
    got = _raw(X, narrow, D, H, side, layout)
    _within(got, ref, f"{n} x {p}, {side}, k = {k}, {layout}: the windows alone")
    among = _raw(X, np.concatenate([narrow[:1], _dense(2, m), narrow[1:]]), D, H, side, layout)
    assert all(v is None or np.array_equal(v, w[[0, 3]]) for v, w in zip(got, among))


# ---- strided rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("side", SIDES)
def test_strided_rows_and_the_scratch(side, layout):
    X = _image(N, "uint8")
    D, H = _model(N, 3)
    W = _mixed(N if side == "pixels" else P)
    assert _same(_raw(X, W, D, H, side, layout, pad=13), _raw(X, W, D, H, side, layout))
    assert _same(_raw(X, W, side=side, layout=layout, pad=13), _raw(X, W, side=side, layout=layout))
    if side == "channels":
        from espm_amd import _lib
        assert _raw(X, W, D, H, side, layout, short=1) == _lib.EINVAL
        need = 3 * 3 * N * 8
        assert f"{need - 1} bytes, {need} needed".encode() in _lib.lib.espm_mu_last_error()


# ---- a second staging round, two pixel chunks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("dtype", ["uint16", "float64"])
@pytest.mark.parametrize("n", [300, 16])
def test_the_other_shapes(n, dtype, side):
    X = _image(n, dtype)
    p = X.shape[1]
    D, H = _model(n, 3)
    m = n if side == "pixels" else p
    W = np.concatenate([_mixed(m), _dense(2, m)])
    W[2, -1] = 1.0   # (the last walk index, alone in its group)
    ref = mr.sums(X, W, D, H, side)
    cm = _raw(X, W, D, H, side, "cm")
    _within(cm, ref, f"{n} x {p}, {dtype}, {side}")
    assert _same(cm, _raw(X, W, D, H, side, "pm"))
    raw = _raw(X, W, side=side)
    _within(raw, mr.sums(X, W, side=side), f"{n} x {p}, {dtype}, {side}, no model")
    assert np.array_equal(raw[0], cm[0]) and _same(raw, _raw(X, W, side=side, layout="pm"))


# ---- line maps ------------------------------------------------------------------------------------------------------------------------------
def test_line_maps(marginals):
    X = _image(N, "uint16")
    D, H = _model(N, 3)
    lines = [((40, 48), ((30, 36), (60, 70))), ((0, 5), None), ((90, 96), ((70, 80), (82, 88))), ((10, 12), ((14, 20), (3, 9)))]
    out = marginals.line_maps(X, lines, D, H)
    U = np.stack([mr.line_weights(N, *line) for line in lines])
    assert np.allclose(out["weights"], U, rtol=0, atol=1e-15)
    U = out["weights"]
    assert np.array_equal(out["net"], marginals.pixel_maps(X, U)["counts"])
    assert np.array_equal(out["net_std"], np.sqrt(marginals.pixel_maps(X, U * U)["counts"]))
    _within((out["net"], None, None), mr.sums(X, U, side="pixels"), "line maps: net")
    _within((out["net_std"] ** 2, None, None), dict(mr.sums(X, U * U, side="pixels"), counts_exact=False,
                                                    counts_bound=mr.gamma(2 * N + 2) * (U * U) @ X.astype(np.float64)), "line maps: net_std^2")
    pm = marginals.line_maps(_lay(X, "pm"), lines, D, H, layout="pm")
    assert all(np.array_equal(out[name], pm[name]) for name in out)
    # the model terms: host products in fp64; the components add up to the modelled line - k products and k - 1 sums against the k
    # multiply-adds of the matrix product: gamma(2 k) of the sum of their magnitudes
    UD = U @ D
    assert np.array_equal(out["model_net"], UD @ H) and out["components"].shape == (4, 3, P)
    assert np.array_equal(out["components"][2, 1], UD[2, 1] * H[1])
    assert (np.abs(out["components"].sum(axis=1) - out["model_net"]) <= mr.gamma(2 * 3) * (np.abs(UD) @ H)).all()
    none = marginals.line_maps(X, lines)
    assert none["model_net"] is None and none["components"] is None and np.array_equal(none["net"], out["net"])
    many = marginals.line_maps(X, lines, *_model(N, 9))   # (no limit of 8 here: the model terms need no pass over X)
    assert many["components"].shape == (4, 9, P) and np.array_equal(many["net"], out["net"])


def test_a_planted_line_is_recovered(marginals):
    """A flat background of 2 counts per channel plus one line of 10 .. 60 counts: the net map is the planted counts within 5 net_std on
    all but LINE_SHARE = 0.5 % of the pixels - a condition on the committed seed that the numpy reference itself keeps
    (tests/test_marginals_cpu.py checks it without a device)."""
    X, planted = mr.planted_line()
    out = marginals.line_maps(X, [mr.LINE])
    u = mr.line_weights(N, *mr.LINE)
    x = X.astype(np.float64)
    assert mr.line_misses(u @ x, np.sqrt((u * u) @ x), planted) <= mr.LINE_SHARE   # the condition
    share = mr.line_misses(out["net"][0], out["net_std"][0], planted)
    print(f"planted line: {share:.4f} of the pixels beyond 5 net_std")
    assert share <= mr.LINE_SHARE
    raw = marginals.line_maps(X, [(mr.LINE[0], None)])
    assert np.array_equal(raw["net"][0], X[40:48].astype(np.int64).sum(axis=0)) and np.array_equal(raw["net_std"][0], np.sqrt(raw["net"][0]))
    assert (raw["net"][0] - planted).mean() > 10   # (without the correction the 16 background counts of the window are in the way)


# ---- the estimator and the adapter ------------------------------------------------------------------------------------------------------------
FN, FSHAPE, FK, FM, DOSE = 64, (24, 24), 3, 7, 1000.0
FP = FSHAPE[0] * FSHAPE[1]


@functools.lru_cache(maxsize=None)
def _problem(m=None):
    from espm_amd import synth
    return synth.make_problem(FN, FSHAPE[0], FSHAPE[1], FK, N=DOSE, seed=2, m=m)


@functools.lru_cache(maxsize=None)
def _specimen(m=None):
    """The 3-phase synthetic spectrum image of tests/test_gpu_attribution.py (espm_amd.synth), 8-bit counts."""
    from espm_amd import synth
    X = synth.sample_numpy(_problem(m), seed=2)
    assert X.max() <= 255
    X = X.astype(np.uint8)
    X.setflags(write=False)
    return X


def _fit(m=None, **kw):
    from espm_amd.estimators import SmoothNMF
    est = SmoothNMF(n_components=FK, simplex_H=True, simplex_W=False, max_iter=30, verbose=0, init="nndsvdar", random_state=0, shape_2d=FSHAPE,
                    G=None if m is None else _problem(m)["G"], **kw)
    X = _specimen(m)
    Xin = np.ascontiguousarray(X.T) if est.hspy_comp else X
    est.fit(Xin.astype(np.float32))
    return est, Xin


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("hspy_comp", [False, True], ids=["cm", "hspy"])
@pytest.mark.parametrize("m", [None, FM], ids=["identity", "dictionary"])
def test_estimator_methods(marginals, m, hspy_comp, normalize):
    from espm_amd import hyperspy_adapter as ha
    est, Xin = _fit(m, hspy_comp=hspy_comp, normalize=normalize)
    kept = {a: np.array(getattr(est, a), copy=True) for a in ("W_", "H_", "G_", "components_", "X_")}
    layout = "pm" if hspy_comp else "cm"
    D, H = est._model_counts()
    n, k, p = FN, FK, FP
    # region spectra of the hard phase map
    labels = np.asarray(est.H_).argmax(axis=0)
    out = est.region_spectra(labels.reshape(FSHAPE), Xin)
    L = int(labels.max()) + 1
    want = marginals.channel_spectra(Xin, mr.label_weights(labels), D, H, log_shift=est.log_shift, layout=layout)
    assert est.region_counts_.shape == est.region_model_.shape == est.region_deviance_.shape == (n, L) and out["counts"] is est.region_counts_
    assert all(np.array_equal(getattr(est, "region_" + name + "_"), want[name]) for name in ("counts", "model", "deviance"))
    assert np.array_equal(est.region_pixels_, np.bincount(labels, minlength=L)) and est.region_pixels_.sum() == p
    diag = est.spectral_diagnostics(Xin)
    assert np.array_equal(est.region_counts_.sum(axis=1), est.sum_spectrum_)   # 8-bit counts: integers all the way
    # the regions' deviances add up to the channel's: the same p terms in another order - the term's roundings and p additions on
    # either side (marginals_reference), and the L - 1 additions here.  (With a dictionary spectral_diagnostics forms G W in fp64 and
    # this method in the fit's fp32: another model, by more than rounding - the spectra themselves are compared with the module's, above.)
    if m is None:
        _, _, _, mag = mr.pieces(_specimen(m), D, H, est.log_shift)
        bound = 2.0 * mr.gamma(2 * mr.term_roundings(k) + 2 * p + L) * mag.sum(axis=1)
        gap = np.abs(est.region_deviance_.sum(axis=1) - diag["channel_deviance"])
        print(f"sum of the regions' deviances against channel_deviance_: worst gap / bound {float((gap / bound).max()):.3g}")
        assert (gap <= bound).all()
    # abundances as soft masks
    soft = est.region_spectra(np.asarray(est.H_, dtype=np.float64) / np.asarray(est.H_, dtype=np.float64).sum(axis=0), Xin)
    assert soft["counts"].shape == (n, k) and np.allclose(soft["pixels"].sum(), p, rtol=1e-12)
    assert np.allclose(soft["counts"].sum(axis=1), est.sum_spectrum_, rtol=1e-12)
    spectra = ha.region_spectra(est)
    assert len(spectra) == 3 and all(s.shape == (k, n) for s in spectra) and np.array_equal(spectra[0], est.region_counts_.T)
    # line maps
    lines = [((20, 28), ((12, 18), (30, 36))), ((40, 44), None)]
    lm = est.line_maps(lines, Xin)
    want = marginals.line_maps(Xin, lines, D, H, layout=layout)
    assert est.lines_.shape == (2, n) and est.line_net_.shape == est.line_net_std_.shape == est.line_model_.shape == (2, p)
    assert est.line_components_.shape == (2, k, p) and lm["net"] is est.line_net_
    for name, attr in (("weights", "lines_"), ("net", "line_net_"), ("net_std", "line_net_std_"), ("model_net", "line_model_"), ("components", "line_components_")):
        assert np.array_equal(getattr(est, attr), want[name]), name
    assert np.array_equal(est.line_net_[1], _specimen(m)[40:44].astype(np.int64).sum(axis=0))
    maps = ha.line_maps(est)
    assert [m.shape for m in maps] == [(2,) + FSHAPE] * 3 + [(2, k) + FSHAPE] and np.array_equal(maps[0].reshape(2, p), est.line_net_)
    for a, v in kept.items():
        assert np.array_equal(np.asarray(getattr(est, a)), v), a


def test_adapter_on_the_raw_cube():
    from espm_amd import hyperspy_adapter as ha
    X = _specimen()
    sig = ha.SpectrumImage(np.ascontiguousarray(X.T).reshape(FSHAPE + (FN,)))
    lines = [((20, 28), ((12, 18), (30, 36))), ((40, 44), None)]
    net, std = sig.line_maps(lines)
    U = np.stack([mr.line_weights(FN, *line) for line in lines])
    ref = mr.sums(X, U, side="pixels")
    assert net.shape == std.shape == (2,) + FSHAPE
    _within((net.reshape(2, FP), None, None), ref, "adapter: line maps")
    assert np.array_equal(net[1].reshape(-1), X[40:44].astype(np.int64).sum(axis=0)) and np.array_equal(std[1], np.sqrt(net[1]))
    labels = (np.arange(FP) % 4 - 1).reshape(FSHAPE)   # -1: no region
    spectra = sig.region_spectra(labels)
    assert spectra.shape == (3, FN)
    for r in range(3):
        assert np.array_equal(spectra[r], X[:, labels.reshape(-1) == r].astype(np.int64).sum(axis=1))


# ---- the wide libraries -----------------------------------------------------------------------------------------------------------------------
def test_the_wide_libraries_have_stubs():
    from espm_amd import _lib
    for k in (12, 20):
        v = _lib.variant(k)
        rc = v.lib.espm_weighted_marginals(None, 0, 0, 8, 8, 8, 0, None, 1, None, None, 0, 1e-14, None, None, None, None, 0, None)
        assert rc == _lib.EUNSUPPORTED and v.lib.espm_weighted_marginals_scratch(1, 96, 1320, 3) == 0
        with pytest.raises(NotImplementedError, match="component library only"):
            v.check(rc)
