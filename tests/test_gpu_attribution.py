"""Count attribution on the device against its numpy restatement (tests/attribution_reference.py): the random split bit for bit -
dtypes, layouts, seeds, component counts, strides, slabs, indices past 2^32, counts the wave shares - the expected attribution within
its derived bound, the estimator's methods against the module, and the adapter's shapes.

The image is the splitting tests' 96 channels x 40 x 33 pixels: 1320 pixels are a ragged last wave and workgroup and two pixel chunks
of the channel side (1024 + 296), 96 channels a ragged block of the channel-per-thread kernels; the model has an all-zero row of D
and two all-zero columns of H."""
import functools

import numpy as np
import pytest

import attribution_reference as ar
import splitting_reference as sr

pytestmark = pytest.mark.gpu

N, SHAPE = 96, (40, 33)
P = SHAPE[0] * SHAPE[1]
SEEDS = [0, (1 << 40) + 3]
KS = [1, 3, 5, 8, 9, 32]
HEAVY = [(3, 64, 256), (17, 700, 300), (48, 660, 65535), (95, 0, 65535), (40, 1319, 257)]   # (what the 16-bit image has planted)


@pytest.fixture(scope="module")
def attribution():
    from espm_amd import attribution
    return attribution


@functools.lru_cache(maxsize=None)
def _model(k):
    D, H = ar.planted_model(N, P, k)
    D.setflags(write=False), H.setflags(write=False)
    return D, H


@functools.lru_cache(maxsize=None)
def _ref_assign(dtype, k, seed):
    parts, invalid = ar.assign(sr.image(N, SHAPE, np.dtype(dtype)), *_model(k), seed)
    parts.setflags(write=False)
    return parts, invalid


@functools.lru_cache(maxsize=None)
def _ref_expected(dtype, k):
    X = sr.image(N, SHAPE, np.uint8 if dtype == "uint8" else np.uint16).astype(dtype)
    return ar.expected(X, *_model(k))


def _lay(X, layout):
    return X if layout == "cm" else np.ascontiguousarray(X.T)


def _lay_parts(parts, layout):
    return parts if layout == "cm" else np.ascontiguousarray(parts.transpose(0, 2, 1))


def _raw_assign(X, D, H, layout, seed, p_total=None, j0=0, pad=0):
    """espm_assign_counts itself on X (n, p) handed over in ``layout``; with ``pad`` the rows of the input and of the k outputs are that
    much longer than they say - the input's padding holds counts that must not be read, the outputs' a fill that must stay.  Returns
    (parts (k, n, p), invalid)."""
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    n, p = X.shape
    k = D.shape[1]
    Xin = _lay(X, layout)
    rows, cols = Xin.shape
    wide = np.full((rows, cols + pad), 201, dtype=X.dtype)
    wide[:, :cols] = Xin
    Xd = torch.from_numpy(wide).to("cuda")
    Dd, Hd = torch.from_numpy(np.ascontiguousarray(D)).to("cuda"), torch.from_numpy(np.ascontiguousarray(H)).to("cuda")
    out = torch.full((k, rows + 1, cols + pad), 77, dtype=Xd.dtype, device="cuda")   # (a spare row between the images)
    cnt = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib.espm_assign_counts(_ptr(Xd), _lib.DIAG_X_U8 if X.dtype == np.uint8 else _lib.DIAG_X_U16,
                                           _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM, cols + pad, n, p, p if p_total is None else p_total,
                                           j0, _ptr(Dd), _ptr(Hd), k, seed, _ptr(out), int(out.stride(0)), cols + pad, _ptr(cnt), _stream()))
    got = out.cpu().numpy()
    assert (got[:, :, cols:] == 77).all() and (got[:, rows, :] == 77).all(), "the padding of the outputs was written"
    got = got[:, :rows, :cols]
    return (got if layout == "cm" else got.transpose(0, 2, 1)), int(cnt.item())


# ---- the random attribution --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
def test_assign_equals_the_rule(attribution, dtype, layout, seed):
    import torch
    X = sr.image(N, SHAPE, np.dtype(dtype))
    D, H = _model(3)
    want, invalid = _ref_assign(dtype, 3, seed)
    parts, info = attribution.assign(_lay(X, layout), D, H, seed=seed, layout=layout)
    assert parts.dtype == X.dtype and parts.shape == (3,) + _lay(X, layout).shape
    assert np.array_equal(parts, _lay_parts(want, layout))
    assert info == dict(invalid=invalid) and invalid > 0
    assert np.array_equal(parts.astype(np.int64).sum(axis=0), _lay(X, layout))
    if dtype == "uint16":   # the entries the wave shares
        for c, j, v in HEAVY:
            got = parts[:, c, j] if layout == "cm" else parts[:, j, c]
            assert int(got.astype(np.int64).sum()) == v and np.array_equal(got, want[:, c, j])
    # two calls are bit-equal; a device tensor is taken where it is and device tensors come back where asked
    T, tinfo = attribution.assign(torch.from_numpy(_lay(X, layout)).to("cuda"), D, H, seed=seed, layout=layout, device=True)
    assert T.is_cuda and T.dtype == getattr(torch, dtype) and np.array_equal(T.cpu().numpy(), parts) and tinfo == info


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("k", KS)
def test_assign_over_the_component_counts(attribution, k, layout):
    X = sr.image(N, SHAPE, np.uint16)
    want, invalid = _ref_assign("uint16", k, SEEDS[1])
    parts, info = attribution.assign(_lay(X, layout), *_model(k), seed=SEEDS[1], layout=layout)
    assert np.array_equal(parts, _lay_parts(want, layout)) and info["invalid"] == invalid
    if k == 1:
        assert np.array_equal(parts[0], _lay(X, layout))


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
def test_assign_with_strided_rows(dtype, layout):
    X = sr.image(N, SHAPE, np.dtype(dtype))
    want, invalid = _ref_assign(dtype, 3, SEEDS[1])
    parts, inv = _raw_assign(X, *_model(3), layout, SEEDS[1], pad=13)
    assert np.array_equal(parts, want) and inv == invalid


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
def test_a_slab_is_its_slice_of_the_whole_attribution(dtype, layout):
    """Pixels 500 .. 819 alone (with the 65535 of pixel 660, the 300 of pixel 700 and the zero column of pixel 500)."""
    X = sr.image(N, SHAPE, np.dtype(dtype))
    D, H = _model(3)
    want, _ = _ref_assign(dtype, 3, SEEDS[1])
    parts, inv = _raw_assign(np.ascontiguousarray(X[:, 500:820]), D, np.ascontiguousarray(H[:, 500:820]), layout, SEEDS[1], p_total=P, j0=500)
    assert np.array_equal(parts, want[:, :, 500:820])
    S = ar.rates(D, H)[-1][:, 500:820]
    assert inv == int(((X[:, 500:820] > 0) & ~(S > 0)).sum())


@pytest.mark.parametrize("layout", ["cm", "pm"])
def test_element_indices_past_2_to_the_32(layout):
    """The last 700 pixels of an image of 2^31 pixels and 4 channels: the indices of channels 2 and 3 need more than 32 bits."""
    p_total, p = 1 << 31, 700
    X = np.ascontiguousarray(sr.image(N, SHAPE, np.uint16)[44:48, 600:1300]).copy()
    X[3, 5], X[2, 699] = 65535, 300
    D, H = sr.model(4, p, 5)
    want, invalid = ar.assign(X, D, H, SEEDS[1], p_total=p_total, j0=p_total - p)
    parts, inv = _raw_assign(X, D, H, layout, SEEDS[1], p_total=p_total, j0=p_total - p)
    assert np.array_equal(parts, want) and inv == invalid
    assert not np.array_equal(want, ar.assign(X, D, H, SEEDS[1])[0])   # (the geometry matters)


# ---- the expected attribution ------------------------------------------------------------------------------------------------------------
def _check_expected(got, ref, what):
    for name, bound in (("pixel_counts", "pixel_bound"), ("ratio_sums", "ratio_bound"), ("counts", "counts_bound")):
        err = np.abs(np.asarray(got[name], dtype=np.float64) - ref[name])
        worst = float((err / np.where(ref[bound] > 0, ref[bound], 1.0)).max())
        print(f"{what}: {name} worst error / bound {worst:.3g}")
        assert (err <= ref[bound]).all(), (what, name, worst)


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32", "float64"])
def test_expected_is_within_the_derived_bound(attribution, dtype):
    X = sr.image(N, SHAPE, np.uint8 if dtype == "uint8" else np.uint16).astype(dtype)
    D, H = _model(3)
    ref = _ref_expected(dtype, 3)
    got = {layout: attribution.expected(_lay(X, layout), D, H, layout=layout) for layout in ("cm", "pm")}
    _check_expected(got["cm"], ref, dtype)
    assert got["cm"]["counts"].dtype == (np.int64 if dtype.startswith("uint") else np.float64)
    again = attribution.expected(X, D, H)
    for name in ("pixel_counts", "ratio_sums", "channel_counts", "counts", "unattributed"):   # the two layouts, and two calls: the same bits
        assert np.array_equal(got["cm"][name], got["pm"][name]), name
        assert np.array_equal(got["cm"][name], again[name]), name
    assert np.array_equal(got["cm"]["channel_counts"], D * got["cm"]["ratio_sums"])
    # nothing is left over but the counts of the planted channel and pixels, whose model is 0
    Xf = X.astype(np.float64)
    left = Xf[20].copy()
    left[[11, 500]] = Xf[:, [11, 500]].sum(axis=0)
    assert left[11] > 0 and left[500] > 0 and left.sum() > 500
    assert (np.abs(got["cm"]["unattributed"] - left) <= ref["identity_bound"]).all()
    assert (np.abs(got["cm"]["channel_counts"].sum(axis=0) - got["cm"]["pixel_counts"].sum(axis=1)) <= ref["totals_bound"]).all()


@pytest.mark.parametrize("k", KS)
def test_expected_over_the_component_counts(attribution, k):
    X = sr.image(N, SHAPE, np.uint16)
    got = attribution.expected(X, *_model(k))
    _check_expected(got, _ref_expected("uint16", k), f"k = {k}")
    pm = attribution.expected(_lay(X, "pm"), *_model(k), layout="pm")
    assert np.array_equal(got["pixel_counts"], pm["pixel_counts"]) and np.array_equal(got["ratio_sums"], pm["ratio_sums"])


# ---- the estimator -----------------------------------------------------------------------------------------------------------------------
FN, FSHAPE, FK, FM, DOSE = 64, (24, 24), 3, 7, 1000.0
FP = FSHAPE[0] * FSHAPE[1]


@functools.lru_cache(maxsize=None)
def _problem(m=None):
    from espm_amd import synth
    return synth.make_problem(FN, FSHAPE[0], FSHAPE[1], FK, N=DOSE, seed=2, m=m)


@functools.lru_cache(maxsize=None)
def _specimen(m=None):
    """A 3-phase synthetic spectrum image (espm_amd.synth), ~15.6 counts per entry: 8-bit counts without an empty line."""
    from espm_amd import synth
    X = synth.sample_numpy(_problem(m), seed=2)
    assert X.max() <= 255 and X.sum(axis=0).min() > 0 and X.sum(axis=1).min() > 0
    X = X.astype(np.uint8)
    X.setflags(write=False)
    return X


def _fit(m=None, **kw):
    from espm_amd.estimators import SmoothNMF
    args = dict(n_components=FK, simplex_H=True, simplex_W=False, max_iter=30, verbose=0, init="nndsvdar", random_state=0, shape_2d=FSHAPE,
                G=None if m is None else _problem(m)["G"])
    args.update(kw)
    est = SmoothNMF(**args)
    X = _specimen(m)
    Xin = np.ascontiguousarray(X.T) if est.hspy_comp else X
    est.fit(Xin.astype(np.float32))
    return est, Xin


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("hspy_comp", [False, True], ids=["cm", "hspy"])
@pytest.mark.parametrize("m", [None, FM], ids=["identity", "dictionary"])
def test_estimator_methods_are_the_module_on_the_fit(attribution, m, hspy_comp, normalize):
    est, Xin = _fit(m, hspy_comp=hspy_comp, normalize=normalize)
    kept = {a: np.array(getattr(est, a), copy=True) for a in ("W_", "H_", "G_", "components_", "X_")}
    layout = "pm" if hspy_comp else "cm"
    W, H = np.asarray(est.W_, dtype=np.float64), np.asarray(est.H_, dtype=np.float64)
    G = np.asarray(est.G_, dtype=np.float64)
    D = W if m is None else G @ W
    n, k, p = FN, FK, FP
    want = attribution.expected(Xin, D, H, log_shift=est.log_shift, layout=layout)
    out = est.attribute_counts(Xin)
    assert np.array_equal(est.pixel_counts_, want["pixel_counts"]) and np.array_equal(est.channel_counts_, want["channel_counts"])
    assert out["pixel_counts"].shape == ((p, k) if hspy_comp else (k, p)) and est.pixel_counts_.shape == (k, p)
    assert est.intensity_W_.shape == est.W_.shape == est.model_intensity_W_.shape
    assert np.array_equal(est.intensity_W_, attribution.intensity(None if m is None else G, W, want["ratio_sums"]))
    assert np.array_equal(est.model_intensity_W_, G.sum(0)[:, None] * W * H.sum(1)[None, :])
    assert np.array_equal(est.component_counts_, want["pixel_counts"].sum(axis=1))
    total = float(Xin.astype(np.int64).sum())
    assert np.array_equal(est.explained_counts_ratio_, est.component_counts_ / total)
    with np.errstate(divide="ignore"):
        assert np.array_equal(est.intensity_rel_error_, 1.0 / np.sqrt(est.intensity_W_))
    assert est.unattributed_counts_ == float(want["unattributed"].sum())
    # the measured counts behind W add up to the attributed total: the chains of attribution_reference's totals_bound, and on top the
    # m roundings of D = G W, the n-term sums of G^T R and the sum over the m k entries
    mm = G.shape[1]
    tb = ar.gamma(2 * k + 2 * n + 2 * p + 2 + 2 * mm + n + mm * k) * est.component_counts_.sum()
    assert abs(est.intensity_W_.sum() - est.component_counts_.sum()) <= tb
    # with the floors of the fit nothing is unattributed beyond the identity's rounding
    assert abs(est.unattributed_counts_) <= ar.gamma(2 * k + n + 2 + p) * total
    # X=None: the fit's X_ un-scaled is the same image up to the roundings of the scaling and the un-scaling in X_'s dtype, and
    # every output is linear in x
    ux = float(np.finfo(np.asarray(est.X_).dtype).eps) / 2
    first = {a: np.array(getattr(est, a), copy=True) for a in ("pixel_counts_", "channel_counts_", "intensity_W_")}
    est.attribute_counts()
    lin = 2 * ux / (1 - 2 * ux) if normalize else 0.0
    for a, rounds in (("pixel_counts_", 2 * (k + n + 2)), ("channel_counts_", 2 * (k + 2) + 2 * p + 1), ("intensity_W_", 2 * (k + 2) + 2 * p + 2 * n + 2)):
        bound = (ar.gamma(rounds) + lin * (1 + ar.gamma(rounds))) * first[a]
        assert (np.abs(getattr(est, a) - first[a]) <= bound).all(), a
    # the random split is the module's, in fit's orientation
    parts = est.assign_counts(Xin, seed=5)
    mod, info = attribution.assign(Xin, D, H, seed=5, layout=layout)
    assert info["invalid"] == 0 and np.array_equal(parts, mod) and parts.shape == (k,) + Xin.shape
    assert np.array_equal(parts.astype(np.int64).sum(axis=0), Xin)
    for a, v in kept.items():
        assert np.array_equal(np.asarray(getattr(est, a)), v), a


def test_measured_intensity_approaches_the_modelled_one_at_a_fixed_point():
    """Unregularised and unconstrained, the multiplicative updates' fixed point has W o (G^T R) = (sum G) W (sum H) entry by entry."""
    gaps = {}
    for iters in (50, 3000):
        est, Xin = _fit(FM, simplex_H=False, simplex_W=False, max_iter=iters, tol=0.0, no_stop_criterion=True)
        est.attribute_counts(Xin)
        gaps[iters] = float(np.abs(est.intensity_W_ - est.model_intensity_W_).sum() / est.model_intensity_W_.sum())
    print(f"relative gap between measured and modelled intensity: {gaps[50]:.3e} after 50 iterations, {gaps[3000]:.3e} after 3000")
    assert gaps[3000] < gaps[50]


def test_adapter_shapes():
    from espm_amd import hyperspy_adapter as ha
    est, Xin = _fit(None, hspy_comp=True)
    with pytest.raises(AttributeError, match="attribute_counts"):
        ha.component_count_maps(est)
    est.attribute_counts(Xin)
    maps, spectra = ha.component_count_maps(est), ha.component_spectra(est)
    assert maps.shape == (FK,) + FSHAPE and np.array_equal(maps.reshape(FK, -1), est.pixel_counts_)
    assert spectra.shape == (FK, FN) and np.array_equal(spectra, est.channel_counts_.T)
    sig = ha.SpectrumImage(Xin.reshape(FSHAPE + (FN,)))
    images = sig.assign_counts(est, seed=3)
    assert len(images) == FK and all(im.data.shape == sig.data.shape and im.data.dtype == np.uint8 for im in images)
    assert np.array_equal(sum(im.data.astype(np.int64) for im in images), sig.data)
    assert np.array_equal(np.stack([im.unfolded() for im in images]), est.assign_counts(Xin, seed=3))
    # an estimator fitted on (channels, pixels) splits the same cube
    est_cm, _ = _fit(None, hspy_comp=False)
    images_cm = sig.assign_counts(est_cm, seed=3)
    assert np.array_equal(np.stack([im.X for im in images_cm]), est_cm.assign_counts(sig.X, seed=3))
