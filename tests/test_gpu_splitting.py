"""Count splitting on the device against its numpy restatement (tests/splitting_reference.py): the thinning kernel bit for bit -
layouts, strides, slabs, indices past 2^32, the extremes of q, counts the wave shares - the two deviances within their derived bound,
``fit_split`` against the pieces it is made of, the scan over the number of components and the adapter's paths.

The image is 96 channels x 40 x 33 pixels: 1320 pixels are no multiple of 64 or 256 (ragged last wave and workgroup of the
deviance kernel), a row of the pixel-major image is a single ragged chunk of the thinning kernel, a row of the channel-major one
a full and a ragged pass of its workgroup."""
import functools

import numpy as np
import pytest

import splitting_reference as sr

pytestmark = pytest.mark.gpu

N, SHAPE = 96, (40, 33)
P = SHAPE[0] * SHAPE[1]
QS = {"half": 0.5, "0.8": 0.8, "least": 2.0 ** -40, "most": 1 - 2.0 ** -40}   # (the last two: thr = 1 and thr = 2^32 - 1)
SEEDS = [0, (1 << 40) + 3]
DTYPES = ["uint8", "uint16"]


@pytest.fixture(scope="module")
def splitting():
    from espm_amd import splitting
    return splitting


@functools.lru_cache(maxsize=None)
def _ref_thin(dtype, thr, seed):
    Xa, Xb = sr.thin(sr.image(N, SHAPE, np.dtype(dtype)), thr, seed)
    Xa.setflags(write=False), Xb.setflags(write=False)
    return Xa, Xb


def _lay(X, layout):
    return X if layout == "cm" else np.ascontiguousarray(X.T)


def _raw_thin(X, layout, thr, seed, p_total=None, j0=0, want_b=True, pad=0):
    """espm_thin_counts itself on X (n, p) handed over in ``layout``; with ``pad`` the rows of input and outputs are that much longer
    than they say - the input's padding holds counts that must not be read, the outputs' a fill that must stay."""
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    n, p = X.shape
    Xin = _lay(X, layout)
    rows, cols = Xin.shape
    wide = np.full((rows, cols + pad), 201, dtype=X.dtype)
    wide[:, :cols] = Xin
    Xd = torch.from_numpy(wide).to("cuda")
    outs = [torch.full((rows, cols + pad), 77, dtype=Xd.dtype, device="cuda") for _ in range(2 if want_b else 1)]
    _lib.check(_lib.lib.espm_thin_counts(_ptr(Xd), _lib.DIAG_X_U8 if X.dtype == np.uint8 else _lib.DIAG_X_U16,
                                         _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM, cols + pad, n, p, p if p_total is None else p_total, j0,
                                         thr, seed, _ptr(outs[0]), _ptr(outs[1]) if want_b else None, cols + pad, _stream()))
    got = [o.cpu().numpy() for o in outs]
    for g in got:
        assert (g[:, cols:] == 77).all(), "the padding of an output row was written"
    got = [g[:, :cols] if layout == "cm" else g[:, :cols].T for g in got]
    return got if want_b else got[0]


# ---- the thinning ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("q", list(QS), ids=list(QS))
@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_thin_equals_the_rule(splitting, dtype, layout, q, seed):
    X = sr.image(N, SHAPE, np.dtype(dtype))
    thr, q_eff = splitting.threshold(QS[q])
    assert (thr, q_eff) == sr.threshold(QS[q])
    Ra, Rb = _ref_thin(dtype, thr, seed)
    Xa, Xb = splitting.thin(_lay(X, layout), q=QS[q], seed=seed, layout=layout)
    assert Xa.dtype == Xb.dtype == X.dtype and Xa.shape == _lay(X, layout).shape
    assert np.array_equal(_lay(Ra, layout), Xa) and np.array_equal(_lay(Rb, layout), Xb)
    assert np.array_equal(Xa.astype(np.int64) + Xb, _lay(X, layout))
    # two calls are bit-equal; device tensors come back where asked, and a device tensor is taken where it is
    import torch
    Ta, Tb = splitting.thin(torch.from_numpy(_lay(X, layout)).to("cuda"), q=QS[q], seed=seed, layout=layout, device=True)
    assert Ta.is_cuda and Ta.dtype == getattr(torch, dtype) and np.array_equal(Ta.cpu().numpy(), Xa) and np.array_equal(Tb.cpu().numpy(), Xb)


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_thin_with_strided_rows_and_without_xb(dtype, layout):
    X = sr.image(N, SHAPE, np.dtype(dtype))
    thr, seed = sr.threshold(0.8)[0], SEEDS[1]
    Ra, Rb = _ref_thin(dtype, thr, seed)
    Xa, Xb = _raw_thin(X, layout, thr, seed, pad=13)
    assert np.array_equal(Xa, Ra) and np.array_equal(Xb, Rb)
    assert np.array_equal(_raw_thin(X, layout, thr, seed, want_b=False, pad=5), Ra)   # xb = NULL


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_slab_is_its_slice_of_the_whole_split(dtype, layout):
    """Pixels 500 .. 819 alone (with the 65535 of pixel 660 and the 300 of pixel 700 in the 16-bit image)."""
    X = sr.image(N, SHAPE, np.dtype(dtype))
    thr, seed = sr.threshold(0.8)[0], SEEDS[1]
    Ra, Rb = _ref_thin(dtype, thr, seed)
    Sa, Sb = _raw_thin(np.ascontiguousarray(X[:, 500:820]), layout, thr, seed, p_total=P, j0=500)
    assert np.array_equal(Sa, Ra[:, 500:820]) and np.array_equal(Sb, Rb[:, 500:820])


@pytest.mark.parametrize("layout", ["cm", "pm"])
def test_element_indices_past_2_to_the_32(layout):
    """The last 700 pixels of an image of 2^31 pixels and 4 channels: the indices of channels 2 and 3 need more than 32 bits."""
    p_total, p = 1 << 31, 700
    X = np.ascontiguousarray(sr.image(N, SHAPE, np.uint16)[44:48, 600:1300])   # (channels 44 .. 47 hold no planted entry but rows of counts)
    X = X.copy()
    X[3, 5], X[2, 699] = 65535, 300
    thr, seed = sr.threshold(0.5)[0], SEEDS[1]
    Ra, Rb = sr.thin(X, thr, seed, p_total=p_total, j0=p_total - p)
    Xa, Xb = _raw_thin(X, layout, thr, seed, p_total=p_total, j0=p_total - p)
    assert np.array_equal(Xa, Ra) and np.array_equal(Xb, Rb)
    assert not np.array_equal(Ra, sr.thin(X, thr, seed, p_total=p, j0=0)[0])   # (the geometry matters)


# ---- the deviances ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_dev(dtype, k):
    thr = sr.threshold(0.8)[0]
    Xa, Xb = _ref_thin(dtype, thr, SEEDS[1])
    D, H = sr.model(N, P, k)
    return D, H, sr.deviances(Xa, Xb, D, H, thr)


@pytest.mark.parametrize("k", [1, 3, 8, 9, 32])
@pytest.mark.parametrize("dtype", DTYPES)
def test_split_deviance(splitting, dtype, k):
    X = sr.image(N, SHAPE, np.dtype(dtype))
    D, H, ref = _ref_dev(dtype, k)
    out = {layout: splitting.split_deviance(_lay(X, layout), D, H, q=0.8, seed=SEEDS[1], layout=layout) for layout in ("cm", "pm")}
    cm = out["cm"]
    for name in ("train", "heldout"):
        err = np.abs(cm[name + "_map"] - ref[name + "_map"])
        print(f"{dtype} k={k} {name}: worst error / bound {float((err / ref[name + '_bound']).max()):.3g}")
        assert np.isfinite(cm[name + "_map"]).all()   # (pixel 11 sits at the log_shift floor)
        assert (err <= ref[name + "_bound"]).all()
        total = float(np.cumsum(ref[name + "_map"])[-1])
        assert abs(cm[name] - total) <= sr.total_bound(ref[name + "_map"], ref[name + "_bound"])
    assert cm["heldout_counts"].dtype == np.int64 and np.array_equal(cm["heldout_counts"], ref["heldout_counts"])
    assert cm["q_eff"] == sr.threshold(0.8)[1]
    # bit-equal across the layouts and across calls
    again = splitting.split_deviance(X, D, H, q=0.8, seed=SEEDS[1])
    for name in ("train_map", "heldout_map", "heldout_counts"):
        assert np.array_equal(cm[name], out["pm"][name]), name
        assert np.array_equal(cm[name], again[name]), name
    assert cm["train"] == out["pm"]["train"] == again["train"] and cm["heldout"] == out["pm"]["heldout"] == again["heldout"]


def test_split_deviance_of_a_slab_with_strided_rows():
    """The entry point itself on pixels 500 .. 819 of the pixel-major 16-bit image, rows 9 entries longer than they say."""
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    k, thr = 3, sr.threshold(0.8)[0]
    D, H, ref = _ref_dev("uint16", k)
    X = sr.image(N, SHAPE, np.uint16)
    wide = np.full((320, N + 9), 999, dtype=np.uint16)
    wide[:, :N] = X[:, 500:820].T
    Xd, Dd, Hd = torch.from_numpy(wide).to("cuda"), torch.from_numpy(D).to("cuda"), torch.from_numpy(np.ascontiguousarray(H[:, 500:820])).to("cuda")
    da, db = (torch.empty(320, dtype=torch.float64, device="cuda") for _ in range(2))
    cb = torch.empty(320, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib.espm_split_deviance(_ptr(Xd), _lib.DIAG_X_U16, _lib.LAYOUT_PM, N + 9, N, 320, P, 500, thr, SEEDS[1], _ptr(Dd), _ptr(Hd), k,
                                            sr.LOG_SHIFT, _ptr(da), _ptr(db), _ptr(cb), _stream()))
    assert np.array_equal(cb.cpu().numpy(), ref["heldout_counts"][500:820])
    assert (np.abs(da.cpu().numpy() - ref["train_map"][500:820]) <= ref["train_bound"][500:820]).all()
    assert (np.abs(db.cpu().numpy() - ref["heldout_map"][500:820]) <= ref["heldout_bound"][500:820]).all()


# ---- fit_split ------------------------------------------------------------------------------------------------------------------------------
FN, FSHAPE, FK, DOSE = 64, (24, 24), 3, 1000.0


@functools.lru_cache(maxsize=None)
def _specimen():
    """A 3-phase synthetic spectrum image (espm_amd.synth), ~15.6 counts per entry, at most 114: 8-bit counts."""
    from espm_amd import synth
    prob = synth.make_problem(FN, FSHAPE[0], FSHAPE[1], FK, N=DOSE, seed=2)
    X = synth.sample_numpy(prob, seed=2)
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


FITS = {"fp32": dict(), "fp64": dict(fp64=True), "hspy_normalize_laplacian": dict(hspy_comp=True, normalize=True, lambda_L=1.0),
        "simplex_W_k2": dict(simplex_H=False, simplex_W=True, n_components=2), "k12": dict(n_components=12)}


@pytest.mark.parametrize("kw", list(FITS.values()), ids=list(FITS))
def test_fit_split_is_its_stages(splitting, kw):
    X = _specimen()
    q, seed = 0.8, 5
    est = _est(**kw)
    Xin = np.ascontiguousarray(X.T) if est.hspy_comp else X
    layout = "pm" if est.hspy_comp else "cm"
    out = est.fit_split(Xin, q=q, seed=seed)
    thr, q_eff = sr.threshold(q)
    Xa, Xb = sr.thin(X, thr, seed)
    # the fit is the fit of the training image
    fresh = _est(**kw)
    ref_out = fresh.fit_transform(_lay(Xa, layout).astype(np.float64 if est._fp64() else np.float32))
    assert np.array_equal(out, ref_out) and np.array_equal(est.W_, fresh.W_) and np.array_equal(est.H_, fresh.H_)
    assert est.n_iter_ == fresh.n_iter_ and est.losses_ == fresh.losses_ and np.array_equal(np.asarray(est.X_), np.asarray(fresh.X_))
    # the attributes
    k = est.H_.shape[0]
    assert est.split_q_ == q_eff and est.split_seed_ == seed
    assert est.train_deviance_map_.shape == est.heldout_deviance_map_.shape == est.heldout_counts_.shape == (X.shape[1],)
    assert np.array_equal(est.heldout_counts_, Xb.sum(axis=0, dtype=np.int64)) and est.heldout_counts_.dtype == np.int64
    D = np.asarray(est.G_ @ est.W_, dtype=np.float64)
    ref = sr.deviances(Xa, Xb, D, np.asarray(est.H_, dtype=np.float64), thr, log_shift=est.log_shift)
    for name in ("train", "heldout"):
        got = getattr(est, name + "_deviance_map_")
        assert (np.abs(got - ref[name + "_map"]) <= ref[name + "_bound"]).all(), name
        bound = sr.total_bound(ref[name + "_map"], ref[name + "_bound"])
        assert abs(getattr(est, name + "_deviance_") - float(np.cumsum(ref[name + "_map"])[-1])) <= bound, name
    if k <= 8:   # the in-sample deviance is the diagnostics' of the training image
        pd = est.pixel_diagnostics(_lay(Xa, layout))["deviance"]
        assert (np.abs(pd - est.train_deviance_map_) <= ref["train_bound"]).all()
        assert abs(est.train_deviance_ - pd.sum()) <= sr.total_bound(ref["train_map"], ref["train_bound"])
    # a later plain fit removes what fit_split set
    est.fit(_lay(Xa, layout).astype(np.float32))
    assert not any(hasattr(est, name) for name in est._SPLIT_ATTRIBUTES)


def test_scan_finds_the_three_phases(splitting):
    """Held-out deviance over n_components = 1 .. 5 on the 3-phase specimen (64 channels, 24 x 24 pixels, dose 1000 counts per pixel:
    15.6 per entry; q = 0.8; simplex_H, no simplex over W, NNDSVDar, 600 iterations, no stop rule).  The numpy fit of the same
    configuration (oracle/mu_oracle.py ``fit`` on the reference split, fp64, CPU) gives

        seed 0: train 60294.8 40963.5 37524.9 36856.6 36051.4   held out 43703.7 39415.4 38958.4 39099.3 39349.9
        seed 1: train 59811.7 40600.2 37286.8 36587.2 35754.1   held out 44189.5 39781.7 39197.0 39377.4 39564.9

    - the minimum at 3 with 457 / 141 (seed 0) and 585 / 180 (seed 1) to its neighbours, a thousand times what separates the fp32
    kernels from that fit; at 300 counts per pixel the minimum moves to 2, at 40 to 1.  The training deviance falls all the way."""
    X = _specimen()
    ests = [_est(n_components=k, max_iter=600, no_stop_criterion=True, tol=0) for k in range(1, 6)]
    out = splitting.scan(X, ests, q=0.8, seeds=(0, 1))
    print("held out", out["heldout"].T, "train", out["train"].T)
    assert out["heldout"].shape == out["train"].shape == (5, 2) and out["q_eff"] == sr.threshold(0.8)[1]
    assert out["best"] == 2
    assert (np.argmin(out["heldout"], axis=0) == 2).all()
    assert (np.diff(out["train"], axis=0) < 0).all()
    assert ests[4].split_seed_ == 1 and ests[4].heldout_deviance_ == out["heldout"][4, 1] and ests[4].H_.shape[0] == 5
    # one estimator of the scan is fit_split of that estimator
    alone = _est(n_components=3, max_iter=600, no_stop_criterion=True, tol=0)
    alone.fit_split(X, q=0.8, seed=1)
    assert alone.heldout_deviance_ == out["heldout"][2, 1] and alone.train_deviance_ == out["train"][2, 1]


# ---- the adapter ------------------------------------------------------------------------------------------------------------------------
def test_adapter_thins_and_decomposes_with_a_split(splitting):
    from espm_amd import hyperspy_adapter as ha
    X = _specimen()
    cube = np.ascontiguousarray(X.T).reshape(*FSHAPE, FN)
    sig = ha.SpectrumImage(cube)
    thr = sr.threshold(0.75)[0]
    Ra, Rb = sr.thin(X, thr, 9)
    A, B = sig.thin(0.75, 9)
    assert isinstance(A, ha.SpectrumImage) and A.data.shape == cube.shape and A.data.dtype == cube.dtype
    assert np.array_equal(A.X, Ra) and np.array_equal(B.X, Rb)
    kw = dict(hspy_comp=True, shape_2d=None)
    est = _est(**kw)
    lr = ha.decompose(sig, est, split=(0.75, 9))
    direct = _est(**kw)
    direct.shape_2d = FSHAPE
    loadings = direct.fit_split(sig.unfolded(), q=0.75, seed=9)
    assert lr.decomposition_algorithm is est and tuple(est.shape_2d) == FSHAPE
    assert np.array_equal(lr.loadings, loadings) and np.array_equal(lr.factors, np.asarray(direct.components_).T)
    assert est.heldout_deviance_ == direct.heldout_deviance_ and est.split_q_ == sr.threshold(0.75)[1] and est.split_seed_ == 9
    assert np.array_equal(est.heldout_counts_, Rb.sum(axis=0, dtype=np.int64))
