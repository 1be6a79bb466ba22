"""Poisson sampling on the device against its numpy restatement (tests/sampling_reference.py): the sampler bit for bit, counters
included - dtypes, layouts, seeds, replicates, component counts, strides, slabs, indices past 2^32, rates the wave shares and rates that
saturate - the null deviance within its derived bound, and ``simulate`` / ``calibrate_deviance`` / ``bootstrap`` against the pieces
they are made of.

The model is 96 channels x 40 x 33 pixels at ~0.6 counts per entry with planted rates (sampling_reference.PLANTED): 1320 pixels are
no multiple of the 256-pixel workgroup, and the pixel-major tile is ragged at 64 + 32 channels."""
import functools

import numpy as np
import pytest

import sampling_reference as sref
import splitting_reference as sr

pytestmark = pytest.mark.gpu

N, SHAPE = 96, (40, 33)
P = SHAPE[0] * SHAPE[1]
SEEDS = [0, (1 << 63) + 12345]
REPLICATES = [0, 7]
DTYPES = ["uint8", "uint16"]


@pytest.fixture(scope="module")
def sampling():
    from espm_amd import sampling
    return sampling


@functools.lru_cache(maxsize=None)
def _model(k=3):
    return sref.model(N, P, k)


@functools.lru_cache(maxsize=None)
def _ref_raw(k, seed, replicate):
    D, H = _model(k)
    raw = sref.raw_rates(sref.rates(D, H), seed, replicate)
    for a in raw:
        a.setflags(write=False)
    return raw


def _ref(k, seed, replicate, dtype):
    return sref.store(_ref_raw(k, seed, replicate), np.dtype(dtype))


def _lay(X, layout):
    return X if layout == "cm" else np.ascontiguousarray(X.T)


def _raw_sample(D, H, seed, replicate, dtype, layout, p_total=None, j0=0, pad=0):
    """espm_poisson_sample itself: (X (n, p), [saturated, invalid]); with ``pad`` the rows of the output are that much longer than they
    say and hold a fill that must stay."""
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    n, k = D.shape
    p = H.shape[1]
    rows, cols = (n, p) if layout == "cm" else (p, n)
    Dd, Hd = torch.from_numpy(np.ascontiguousarray(D)).to("cuda"), torch.from_numpy(np.ascontiguousarray(H)).to("cuda")
    out = torch.full((rows, cols + pad), 77, dtype=getattr(torch, dtype), device="cuda")
    counts = torch.full((2,), -5, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib.espm_poisson_sample(_ptr(Dd), _ptr(Hd), k, n, p, p if p_total is None else p_total, j0, seed, replicate, _ptr(out),
                                            _lib.DIAG_X_U8 if dtype == "uint8" else _lib.DIAG_X_U16,
                                            _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM, cols + pad, _ptr(counts), _stream()))
    got = out.cpu().numpy()
    assert (got[:, cols:] == 77).all(), "the padding of an output row was written"
    got = got[:, :cols]
    return (got if layout == "cm" else got.T), counts.cpu().numpy().tolist()


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------------
def test_the_planted_rates_are_exact():
    D, H = _model()
    y = sref.rates(D, H)
    for c, j, rate, d in sref.PLANTED:
        assert y[c, j] == rate
    assert (y[:, 11] == 0).all() and ((y >= 256) & (y <= 65535)).sum() > 20 and (y > 65535).sum() >= 1
    X, info = _ref(3, 0, 0, "uint16")
    assert X[2, 20] == 0 and X[4, 70] == 0 and X[18, 800] == 65535 and info["saturated"] >= 1 and info["invalid"] == 0


@pytest.mark.parametrize("replicate", REPLICATES)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sample_equals_the_rule(sampling, dtype, layout, seed, replicate):
    D, H = _model()
    R, rinfo = _ref(3, seed, replicate, dtype)
    X, info = sampling.sample(D, H, seed=seed, replicate=replicate, dtype=np.dtype(dtype), layout=layout)
    assert X.dtype == np.dtype(dtype) and X.shape == _lay(R, layout).shape
    assert np.array_equal(X, _lay(R, layout))
    assert info == rinfo and info["invalid"] == 0
    if dtype == "uint8":   # 8 bits saturate at 255, with the count the reference gives
        assert X.max() == 255 and info["saturated"] == int((np.minimum(_ref_raw(3, seed, replicate)[0], 256) > 255).sum() +
                                                           _ref_raw(3, seed, replicate)[2].sum()) > 20
    # two calls are bit-equal; a device tensor comes back where asked, with the host path's values
    import torch
    T, tinfo = sampling.sample(D, H, seed=seed, replicate=replicate, dtype=np.dtype(dtype), layout=layout, device=True)
    assert T.is_cuda and T.dtype == getattr(torch, dtype) and np.array_equal(T.cpu().numpy(), X) and tinfo == info


@pytest.mark.parametrize("k,layout,dtype", [(1, "cm", "uint16"), (3, "pm", "uint16"), (8, "pm", "uint8"), (9, "cm", "uint8"), (32, "pm", "uint16")])
def test_sample_over_the_component_counts(sampling, k, layout, dtype):
    """k = 1 (of KP = 4), 3, 8 (the whole of KP = 8), 9 (KP = 16) and 32."""
    D, H = _model(k)
    R, rinfo = _ref(k, 5, 2, dtype)
    X, info = sampling.sample(D, H, seed=5, replicate=2, dtype=np.dtype(dtype), layout=layout)
    assert np.array_equal(X, _lay(R, layout)) and info == rinfo


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sample_with_strided_rows(dtype, layout):
    D, H = _model()
    R, rinfo = _ref(3, SEEDS[1], 7, dtype)
    X, counts = _raw_sample(D, H, SEEDS[1], 7, dtype, layout, pad=13)
    assert np.array_equal(X, R) and counts == [rinfo["saturated"], rinfo["invalid"]]


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_slab_is_its_slice_of_the_whole_sample(dtype, layout):
    """Pixels 256 .. 555 alone (with the 255.5 of pixel 300, the 256.0 of pixel 400 and the 300.25 of pixel 500)."""
    D, H = _model()
    raw = _ref_raw(3, SEEDS[1], 7)
    R, rinfo = sref.store(tuple(a[:, 256:556] for a in raw), np.dtype(dtype))
    X, counts = _raw_sample(D, H[:, 256:556], SEEDS[1], 7, dtype, layout, p_total=P, j0=256)
    assert np.array_equal(X, R) and counts == [rinfo["saturated"], rinfo["invalid"]]


@pytest.mark.parametrize("layout", ["cm", "pm"])
def test_element_indices_past_2_to_the_32(layout):
    """The last 700 pixels of an image of 2^33 pixels and 4 channels (16 .. 19 of the model, with the 65535.0 and the 65536.5 among
    pixels 600 .. 1299): every index of channels 1 .. 3 needs more than 32 bits."""
    p_total, p = 1 << 33, 700
    D, H = _model()
    D, H = np.ascontiguousarray(D[16:20]), np.ascontiguousarray(H[:, 600:1300])
    R, rinfo = sref.sample(D, H, SEEDS[1], 3, p_total=p_total, j0=p_total - p)
    X, counts = _raw_sample(D, H, SEEDS[1], 3, "uint16", layout, p_total=p_total, j0=p_total - p)
    assert np.array_equal(X, R) and counts == [rinfo["saturated"], rinfo["invalid"]] and rinfo["saturated"] >= 1
    assert not np.array_equal(R, sref.sample(D, H, SEEDS[1], 3)[0])   # (the geometry matters)


@pytest.mark.parametrize("layout", ["cm", "pm"])
def test_invalid_rates_are_zero_and_counted(layout):
    """The entry point itself with one negative entry of d: the rates of channel 20 fall below zero wherever component 1 weighs
    enough - those entries are 0 and counted, the others are drawn as ever."""
    D, H = _model()
    D = D.copy()
    D[20, 1] = -3.0
    R, rinfo = sref.sample(D, H, 9, 1)
    assert 100 < rinfo["invalid"] < P and (R[20] > 0).any()
    for dtype in DTYPES:
        Rd, rinfo = sref.sample(D, H, 9, 1, dtype=np.dtype(dtype))
        X, counts = _raw_sample(D, H, 9, 1, dtype, layout)
        assert np.array_equal(X, Rd) and counts == [rinfo["saturated"], rinfo["invalid"]]
    again = _raw_sample(D, H, 9, 1, "uint16", layout)
    assert np.array_equal(again[0], R) and again[1] == counts   # two calls: the same values, the same counters


# ---- the null deviance ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_null(k, seed, replicate0, n_rep):
    D, H = _model(k)
    return [sref.deviance(_ref(k, seed, replicate0 + r, "uint16")[0], D, H) for r in range(n_rep)]


@pytest.mark.parametrize("k", [3, 12])
def test_null_deviance_is_the_deviance_of_the_replicates(sampling, k):
    """Replicates 5, 6, 7 of seed 0; pixel 11 sits at the log_shift floor, pixel 800 holds the saturated entry (65535 against
    65536.5)."""
    D, H = _model(k)
    ref = _ref_null(k, 0, 5, 3)
    got = sampling.null_deviance(D, H, n_rep=3, seed=0, replicate0=5)
    assert got.shape == (3, P) and got.dtype == np.float64 and np.isfinite(got).all()
    for r in range(3):
        err = np.abs(got[r] - ref[r]["map"])
        print(f"k={k} replicate {5 + r}: worst error / bound {float((err / ref[r]['bound']).max()):.3g}")
        assert (err <= ref[r]["bound"]).all()
    assert abs(got[0, 11] - 2 * N * sr.LOG_SHIFT) <= ref[0]["bound"][11]
    assert np.array_equal(got, sampling.null_deviance(D, H, n_rep=3, seed=0, replicate0=5))   # two calls give the same bits
    # a row is a row of any call that holds the replicate
    assert np.array_equal(got[2], sampling.null_deviance(D, H, n_rep=2, seed=0, replicate0=7)[0])


def test_null_deviance_agrees_with_the_pixel_diagnostics(sampling):
    """measures.pixel_diagnostics of the materialised replicate 7: within the sum of the two derived bounds (its own:
    tests/diag_reference.py, 8 n eps sum_c |t_c|)."""
    from espm_amd import measures
    D, H = _model()
    ref = _ref_null(3, 0, 5, 3)[2]
    X = _ref(3, 0, 7, "uint16")[0]
    pd = measures.pixel_diagnostics(X, D, H, log_shift=sr.LOG_SHIFT)["deviance"]
    got = sampling.null_deviance(D, H, n_rep=1, seed=0, replicate0=7)[0]
    bound = ref["bound"] + 8 * N * sref.EPS * ref["abs_terms"]
    print(f"null deviance against pixel_diagnostics: worst difference / bound {float((np.abs(got - pd) / bound).max()):.3g}")
    assert (np.abs(got - pd) <= bound).all()


# ---- the estimator -------------------------------------------------------------------------------------------------------------------------
FN, FSHAPE, FK, DOSE = 64, (24, 24), 3, 1000.0
FP = FSHAPE[0] * FSHAPE[1]


@functools.lru_cache(maxsize=None)
def _problem(m=None):
    from espm_amd import synth
    return synth.make_problem(FN, FSHAPE[0], FSHAPE[1], FK, N=DOSE, seed=2, m=m)


@functools.lru_cache(maxsize=None)
def _specimen():
    """A 3-phase synthetic spectrum image (espm_amd.synth), ~15.6 counts per entry, at most 114: 8-bit counts."""
    from espm_amd import synth
    X = synth.sample_numpy(_problem(), seed=2)
    assert X.max() <= 255
    X = X.astype(np.uint8)
    X.setflags(write=False)
    return X


def _est(**kw):
    from espm_amd.estimators import SmoothNMF
    fp64 = kw.pop("fp64", False)
    args = dict(n_components=FK, simplex_H=True, simplex_W=False, max_iter=40, verbose=0, init="nndsvdar", random_state=0, shape_2d=FSHAPE)
    args.update(kw)
    est = SmoothNMF(**args)
    return est.set_precision("fp64") if fp64 else est


def _fit(**kw):
    est = _est(**kw)
    X = _specimen()
    est.fit((np.ascontiguousarray(X.T) if est.hspy_comp else X).astype(np.float64 if est._fp64() else np.float32))
    return est


FITS = {"fp32": dict(), "hspy_normalize_laplacian": dict(hspy_comp=True, normalize=True, lambda_L=1.0)}


@pytest.mark.parametrize("kw", list(FITS.values()), ids=list(FITS))
def test_simulate_is_a_sample_of_the_fitted_model(sampling, kw):
    est = _fit(**kw)
    layout = "pm" if est.hspy_comp else "cm"
    D, H = np.asarray(est.G_ @ est.W_, dtype=np.float64), np.asarray(est.H_, dtype=np.float64)
    assert abs((D @ H).sum() / _specimen().sum() - 1) < 0.05   # (count units, whatever normalize was)
    X = est.simulate(seed=4, replicate=2)
    assert X.dtype == np.uint16 and X.shape == ((FP, FN) if est.hspy_comp else (FN, FP))
    S, info = sampling.sample(D, H, seed=4, replicate=2, layout=layout)
    R, rinfo = sref.sample(D, H, 4, 2)
    assert info == rinfo == dict(saturated=0, invalid=0)
    assert np.array_equal(X, S) and np.array_equal(X, _lay(R, layout))
    T = est.simulate(seed=4, replicate=2, device=True)
    assert T.is_cuda and np.array_equal(T.cpu().numpy(), X)
    assert not np.array_equal(est.simulate(seed=4, replicate=3), X)
    # the adapter hands it over as a spectrum image
    from espm_amd import hyperspy_adapter as ha
    sig = ha.SpectrumImage.simulate(est, seed=4, replicate=2)
    assert sig.data.shape == FSHAPE + (FN,) and np.array_equal(sig.X, R)


def test_simulate_refuses_a_saturated_replicate(sampling):
    est = _fit()
    est.W_ = est.W_ * 1e4   # (rates far above 65535)
    with pytest.raises(ValueError, match="saturated"):
        est.simulate()


@pytest.mark.parametrize("kw", list(FITS.values()), ids=list(FITS))
def test_calibrate_deviance_is_its_stages(sampling, kw):
    est = _fit(**kw)
    X = _specimen()
    Xin = np.ascontiguousarray(X.T) if est.hspy_comp else X
    out = est.calibrate_deviance(Xin, n_rep=20, seed=6)
    D, H = np.asarray(est.G_ @ est.W_, dtype=np.float64), np.asarray(est.H_, dtype=np.float64)
    fresh = _fit(**kw)
    dev = fresh.pixel_diagnostics(Xin)["deviance"]
    null = sampling.null_deviance(D, H, n_rep=20, seed=6, replicate0=0, log_shift=est.log_shift)
    cal = sampling.calibrate(dev, null)
    assert np.array_equal(est.deviance_, dev) and np.array_equal(est.H_std_, fresh.H_std_, equal_nan=True)
    for name, key in (("deviance_null_mean_", "null_mean"), ("deviance_null_std_", "null_std"), ("deviance_z_", "z"), ("deviance_pvalue_", "pvalue")):
        assert getattr(est, name).shape == (FP,) and np.array_equal(getattr(est, name), cal[key]) and np.array_equal(out[key], cal[key]), name
    assert est.deviance_null_rep_ == 20 and np.array_equal(out["deviance"], dev)
    # row r of the null is the deviance of simulate(seed, r)
    ref = sref.deviance(sref.sample(D, H, 6, 3)[0], D, H, log_shift=est.log_shift)
    assert (np.abs(null[3] - ref["map"]) <= ref["bound"]).all()
    from espm_amd import hyperspy_adapter as ha
    z, pv = ha.calibrated_deviance_maps(est)
    assert z.shape == pv.shape == FSHAPE and np.array_equal(z.ravel(), est.deviance_z_)


CAL_DOSE, CAL_IMAGE_SEED, CAL_NULL_SEED, CAL_PIXEL = 60.0, 11, 12, 100


def _known_model():
    """The specimen's own model at 60 counts per pixel (0.94 per entry), and an estimator that holds it as its fit."""
    prob = _problem()
    D = CAL_DOSE * np.asarray(prob["phases"], dtype=np.float64).T
    H = np.ascontiguousarray(np.asarray(prob["weights"], dtype=np.float64).T)
    est = _est()
    est.G_, est.W_, est.H_, est._identity_G = np.eye(FN), D, H, True
    return prob, D, H, est


def test_calibrated_deviance_is_standard_under_the_model_and_flags_a_foreign_pixel():
    """An image drawn by the rule (seed 11) from a known model, calibrated against that model with 200 replicates of seed 12.  Under
    the model z is standardised: |mean| <= 5 / sqrt(p), standard deviation in [0.8, 1.25].  Pixel 100 with the spectrum of another
    phase at double dose lies above all 200 null replicates: p = 1 / 201; in the unmodified image its p-value is above 0.01.  All
    seeds are fixed: the numpy reference gives, for these seeds, mean(z) = -0.0044 (limit 0.2083), std(z) = 1.0026, and for pixel 100
    p = 0.70 unmodified and 1 / 201 modified (its deviance 220.4 against a largest null value of 86.2)."""
    prob, D, H, est = _known_model()
    y = sref.rates(D, H)
    X, info = sref.sample_rates(y, CAL_IMAGE_SEED, 0)
    assert info == dict(saturated=0, invalid=0)
    out = est.calibrate_deviance(X, n_rep=200, seed=CAL_NULL_SEED)
    z = out["z"]
    print(f"z: mean {z.mean():+.4f} (limit {5 / np.sqrt(FP):.4f}), std {z.std(ddof=1):.4f}; pixel {CAL_PIXEL}: p = {out['pvalue'][CAL_PIXEL]:.4f}")
    assert abs(z.mean()) <= 5 / np.sqrt(FP)
    assert 0.8 <= z.std(ddof=1) <= 1.25
    assert out["pvalue"][CAL_PIXEL] > 0.01
    other = (int(np.argmax(H[:, CAL_PIXEL])) + 1) % FK
    y2 = y.copy()
    y2[:, CAL_PIXEL] = 2 * CAL_DOSE * prob["phases"][other]
    X2 = X.copy()
    X2[:, CAL_PIXEL] = sref.sample_rates(y2, CAL_IMAGE_SEED, 0)[0][:, CAL_PIXEL]
    out2 = est.calibrate_deviance(X2, n_rep=200, seed=CAL_NULL_SEED)
    print(f"modified pixel: deviance {out2['deviance'][CAL_PIXEL]:.2f}, null mean {out2['null_mean'][CAL_PIXEL]:.2f}, z {out2['z'][CAL_PIXEL]:.2f}")
    assert out2["pvalue"][CAL_PIXEL] == 1 / 201
    assert np.array_equal(out2["null_mean"], out["null_mean"])   # (the same null: it depends on the model and the seed alone)


# ---- the bootstrap ------------------------------------------------------------------------------------------------------------------------
def _dictionary():
    return np.asarray(_problem(17)["G"], dtype=np.float64)


BOOTS = {"fp32": dict(), "hspy_normalize_laplacian": dict(hspy_comp=True, normalize=True, lambda_L=1.0), "fp64": dict(fp64=True),
         "dictionary_G": dict(G="dictionary", simplex_W=False)}


@pytest.mark.parametrize("kw", list(BOOTS.values()), ids=list(BOOTS))
def test_bootstrap_is_its_refits(sampling, kw):
    from sklearn.base import clone
    kw = dict(kw)
    if kw.get("G") == "dictionary":
        kw["G"] = _dictionary()
    est = _fit(**kw)
    before = dict(W=est.W_, H=est.H_, X=est.X_, losses=est.losses_, n_iter=est.n_iter_)
    copies = dict(W=est.W_.copy(), H=est.H_.copy(), losses=list(est.losses_))
    out = est.bootstrap(n_boot=3, seed=8, max_iter=30, return_samples=True)
    # the estimator's own fit is untouched
    assert est.W_ is before["W"] and est.H_ is before["H"] and est.X_ is before["X"] and est.losses_ is before["losses"]
    assert np.array_equal(est.W_, copies["W"]) and np.array_equal(est.H_, copies["H"]) and est.losses_ == copies["losses"]
    assert est.n_iter_ == before["n_iter"] and est.max_iter == 40
    # replicate r is a hand-made copy fitted on simulate(seed, r) from the same start
    W0 = est.W_ * est.norm_factor_ if est.normalize else est.W_
    Ws, Hs, Ds = [], [], []
    for r in range(3):
        hand = clone(est)
        hand.max_iter = 30
        if est._fp64():
            hand.set_precision("fp64")
        hand.fit_transform(est.simulate(seed=8, replicate=r).astype(np.float64 if est._fp64() else np.float32), W=W0.copy(), H=est.H_.copy())
        assert np.array_equal(out["W_samples"][r], hand.W_) and np.array_equal(out["H_samples"][r], hand.H_), r
        assert hand.n_iter_ <= 30
        Ws.append(np.asarray(hand.W_, dtype=np.float64)), Hs.append(np.asarray(hand.H_, dtype=np.float64))
        Ds.append(np.asarray(hand.G_, dtype=np.float64) @ Ws[-1])
    assert not np.array_equal(Ws[0], Ws[1])
    # means and standard deviations (ddof = 1) of the three; either formula is good to a few eps of the mean
    for name, vals in (("W", Ws), ("H", Hs)):
        scale = 1e-12 * np.abs(np.mean(vals, axis=0)).max()
        np.testing.assert_allclose(getattr(est, name + "_boot_mean_"), np.mean(vals, axis=0), rtol=1e-12, atol=scale)
        np.testing.assert_allclose(getattr(est, name + "_boot_std_"), np.std(vals, axis=0, ddof=1), rtol=1e-12, atol=scale)
    np.testing.assert_allclose(est.D_boot_std_, np.std(Ds, axis=0, ddof=1), rtol=1e-12, atol=1e-12 * np.abs(Ds[0]).max())
    k = est.H_.shape[0]
    assert est.W_boot_mean_.shape == est.W_boot_std_.shape == est.W_.shape
    assert est.H_boot_mean_.shape == est.H_boot_std_.shape == (k, FP) and est.D_boot_std_.shape == (FN, k)   # (as H_ and G_ W_, with hspy_comp too)
    assert est.n_boot_ == 3 and est.boot_seed_ == 8 and out["H_std"] is est.H_boot_std_
    assert (est.H_boot_std_ > 0).any() and np.isfinite(est.H_boot_std_).all()
    from espm_amd import hyperspy_adapter as ha
    assert ha.bootstrap_maps(est).shape == (k,) + FSHAPE
    # the Cramer-Rao bound next to it (recorded, not asserted: nobody knows their ratio under regularisation)
    if not est._fp64() and kw.get("G") is None:
        est.pixel_diagnostics()
        print(f"median H_boot_std_ / H_std_ (3 replicates, 30 iterations): {np.nanmedian(est.H_boot_std_ / est.H_std_):.3f}")


def test_bootstrap_refuses_before_upload(sampling, monkeypatch):
    X = _specimen()
    uploads = []
    real = sampling._upload
    monkeypatch.setattr(sampling, "_upload", lambda *a, **k: (uploads.append(1), real(*a, **k))[1])
    binned = _est()
    binned.fit_binned(X, (2, 2))
    for call in (lambda e: e.bootstrap(n_boot=2), lambda e: e.simulate(), lambda e: e.calibrate_deviance(X)):
        with pytest.raises(ValueError, match="fit_binned"):
            call(binned)
        sharded = _fit()
        sharded.shard(object())
        with pytest.raises(NotImplementedError, match="shard"):
            call(sharded)
    assert not uploads
    _fit().simulate()
    assert len(uploads) == 1   # (the counter counts)
