"""Pixel binning on the GPU (csrc/mu_binning.hip, espm_amd/binning.py, NMFEstimator.fit_binned) against the numpy reference of
tests/binning_reference.py.

Shapes: the smallest at which edges, ragged bins and block boundaries all occur - images of 13 x 10 (ragged in both directions),
16 x 24 (dividing), 37 x 67 pixels (2479: more than a 2048-pixel chunk, a row longer than a wave) and 3 x 530 (wider than two
256-column strips of the channel-major kernel, with bins up to and beyond a strip), 70 and 256 + 52 channels (one
and five blocks of 64 channels, neither a multiple), bins from (1, 1) to one that is larger than every image, the four dtypes, both
layouts, one case with a row stride above the row length.

Bounds.  Integer bin sums are exact.  A floating-point bin sum is a sum of at most by bx non-negative terms in fp64, rounded once
to the output: within by bx eps(output) of the reference, relative, per entry.  T1, T2, A and C are sums of non-negative terms, so
each is within (terms + 4) 2^-52, relative, of the reference whatever the order: terms = n p for T1 and T2, n x (bins of the grid)
for A and C.  The risk is a combination of the four in which the bias cancels: within the candidate's bound times
(T2 + T1 + A + C) / (K L), absolute."""
import functools

import numpy as np
import pytest

import binning_reference as br

pytestmark = pytest.mark.gpu

IMAGES = [(13, 10), (16, 24), (37, 67)]
CHANNELS = [70, 256 + 52]
BINS = [(1, 1), (2, 2), (3, 4), (5, 5), (4, 1), (1, 8), (64, 128)]
DTYPES = ["uint8", "uint16", "float32", "float64"]
U = 2.0 ** -52


# an image wider than two 256-column strips of the channel-major kernel: second and ragged last strips ((1, 1): 256 + 256 + 18;
# (2, 7): strips of 36 bins, 252 columns), a bin as wide as a strip, bins wider than one ((2, 300) with a ragged second bin, (1, 1000):
# the whole row in three pieces), and the pixel-major row walk with its slabs on wide bins
WIDE = (3, 530)
WIDE_BINS = [(1, 1), (2, 7), (1, 256), (2, 300), (1, 1000)]


def _bins(shape):
    if shape == WIDE:
        return WIDE_BINS
    return BINS + ([(16, 3)] if shape == (13, 10) else [])   # (16, 3) on 13 x 10: one bin row


@pytest.fixture(scope="module")
def binning():
    from espm_amd import binning
    return binning


@functools.lru_cache(maxsize=None)
def _image(n, shape, dtype):
    """(n, ny nx) counts with a spatial structure, an empty pixel and an empty channel; u16 holds counts far above 255, the float
    images values that are no integers."""
    rng = np.random.default_rng(1000 * n + 10 * shape[0] + len(dtype))
    p = shape[0] * shape[1]
    lam = rng.gamma(1.0, 2.0, size=(n, 1)) * (0.2 + rng.random((1, p)))
    X = rng.poisson(lam).astype(np.float64)
    if dtype == "uint16":
        X[rng.random(X.shape) < 0.05] *= 3000.0
        X = np.minimum(X, 65535)
    elif dtype == "uint8":
        X = np.minimum(X, 255)
    else:
        X = X * 0.37 + rng.random(X.shape) * (X > 0)
    X[:, p // 3] = 0
    X[n // 2] = 0
    X = X.astype(dtype)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _ref_sums(n, shape, dtype):
    return br.sums(_image(n, shape, dtype), shape, _bins(shape))


def _as_input(X, layout, padded=False):
    import torch
    Xin = X if layout == "cm" else np.ascontiguousarray(X.T)
    if padded:   # rows 12 elements longer than they say, filled with counts that must not be read
        wide = np.full((Xin.shape[0], Xin.shape[1] + 12), 255 if Xin.dtype == np.uint8 else 999, dtype=Xin.dtype)
        wide[:, :Xin.shape[1]] = Xin
        Xin = torch.from_numpy(wide).to("cuda")[:, :Xin.shape[1]]
        assert Xin.stride(0) == wide.shape[1]
    return Xin


def _check_rebin(binning, X, shape, layout, padded=False):
    Xin = _as_input(X, layout, padded)
    integer = X.dtype.kind == "u"
    for bin in _bins(shape):
        out = binning.rebin(Xin, shape, bin, layout=layout)
        again = binning.rebin(Xin, shape, bin, layout=layout)
        assert out.dtype == again.dtype and np.array_equal(out, again), f"{bin}: two calls differ"
        got = out if layout == "cm" else out.T
        gny, gnx = br.grid(shape, bin)
        assert got.shape == (X.shape[0], gny * gnx), bin
        B = min(bin[0], shape[0]) * min(bin[1], shape[1])
        if integer:
            ref = br.rebin_exact(X, shape, bin)
            assert out.dtype == (np.float32 if int(X.max()) * B < 2 ** 24 else np.float64), bin
            assert np.array_equal(got.astype(np.float64), ref.astype(np.float64)), f"{bin}: integer bin sums are exact"
        else:
            ref, _ = br.rebin(X, shape, bin)
            assert out.dtype == X.dtype, bin
            err = np.abs(got.astype(np.float64) - ref)
            tol = bin[0] * bin[1] * float(np.finfo(out.dtype).eps) * ref
            worst = float((err / np.maximum(tol, 1e-300)).max())
            print(f"rebin {shape} n={X.shape[0]} {X.dtype} {layout} {bin}: worst error / bound {worst:.3g}")
            assert (err <= tol).all(), bin
        if bin == (1, 1):
            assert np.array_equal(got.astype(np.float64), np.asarray(X, dtype=np.float64)), "(1, 1) returns the values unchanged"


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", CHANNELS)
@pytest.mark.parametrize("shape", IMAGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rebin_parity(binning, shape, n, dtype, layout):
    _check_rebin(binning, _image(n, shape, dtype), shape, layout)


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rebin_parity_wide_image(binning, dtype, layout):
    _check_rebin(binning, _image(70, WIDE, dtype), WIDE, layout)


@pytest.mark.parametrize("layout", ["cm", "pm"])
def test_rebin_writes_rows_out_ld_apart(layout):
    """The entry point itself with an output whose rows are 5 elements longer than they say: the padding keeps its fill."""
    import torch

    from espm_amd import _lib
    from espm_amd.engine import _ptr, _stream
    shape, bin, n = (13, 10), (3, 4), 70
    X = _image(n, shape, "uint16")
    Xd = torch.from_numpy(np.array(X if layout == "cm" else X.T, order="C")).to("cuda")
    gny, gnx = br.grid(shape, bin)
    rows, cols = (n, gny * gnx) if layout == "cm" else (gny * gnx, n)
    out = torch.full((rows, cols + 5), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib.espm_rebin_pixels(_ptr(Xd), _lib.DIAG_X_U16, _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM, int(Xd.stride(0)), n,
                                          shape[0], shape[1], bin[0], bin[1], _ptr(out), _lib.DIAG_X_F64, int(out.stride(0)), _stream()))
    got = out.cpu().numpy()
    ref = br.rebin_exact(X, shape, bin).astype(np.float64)
    assert np.array_equal(got[:, :cols], ref if layout == "cm" else ref.T)
    assert (got[:, cols:] == -7.0).all()


@pytest.mark.parametrize("layout,dtype", [("cm", "uint8"), ("pm", "float32"), ("cm", "uint16"), ("pm", "float64")])
def test_rebin_reads_no_padding(binning, layout, dtype):
    _check_rebin(binning, _image(70, (37, 67), dtype), (37, 67), layout, padded=True)


def _sum_bounds(n, shape, bins):
    p = shape[0] * shape[1]
    return (n * p + 4) * U, np.array([(n * br.n_bins_in_grid(shape, (min(b[0], shape[0]), min(b[1], shape[1]))) + 4) * U for b in bins])


def _check_sums(binning, X, shape, layout, ref, padded=False):
    n, bins = X.shape[0], _bins(shape)
    Xin = _as_input(X, layout, padded)
    T1, T2, A, Cs = binning.binning_sums(Xin, shape, bins, layout=layout)
    again = binning.binning_sums(Xin, shape, bins, layout=layout)
    assert (T1, T2) == again[:2] and np.array_equal(A, again[2]) and np.array_equal(Cs, again[3]), "two calls differ"
    r1, r2, rA, rC = ref
    bT, bA = _sum_bounds(n, shape, bins)
    tag = f"sums {shape} n={n} {X.dtype} {layout}"
    print(f"{tag}: T1 {abs(T1 - r1) / r1 / bT:.3g} T2 {abs(T2 - r2) / r2 / bT:.3g} A {(np.abs(A - rA) / rA / bA).max():.3g} "
          f"C {(np.abs(Cs - rC) / rC / bA).max():.3g} of their bounds")
    assert abs(T1 - r1) <= bT * r1 and abs(T2 - r2) <= bT * r2
    assert (np.abs(A - rA) <= bA * rA).all() and (np.abs(Cs - rC) <= bA * rC).all()
    risk = binning.risk_from_sums(T1, T2, A, Cs, n, *shape)[2]
    rrisk = br.risk(r1, r2, rA, rC, n, shape)[2]
    scale = (r2 + r1 + rA + rC) / (n * shape[0] * shape[1])
    print(f"{tag}: risk error / bound {(np.abs(risk - rrisk) / (bA * scale)).max():.3g}")
    assert (np.abs(risk - rrisk) <= bA * scale).all()
    return T1, T2, A, Cs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", CHANNELS)
@pytest.mark.parametrize("shape", IMAGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_binning_sums_parity(binning, shape, n, dtype):
    X, ref = _image(n, shape, dtype), _ref_sums(n, shape, dtype)
    cm = _check_sums(binning, X, shape, "cm", ref)
    pm = _check_sums(binning, X, shape, "pm", ref)
    bT, bA = _sum_bounds(n, shape, _bins(shape))   # the two layouts: within the bound of each other
    assert abs(cm[0] - pm[0]) <= bT * cm[0] and abs(cm[1] - pm[1]) <= bT * cm[1]
    assert (np.abs(cm[2] - pm[2]) <= bA * cm[2]).all() and (np.abs(cm[3] - pm[3]) <= bA * cm[3]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_binning_sums_parity_wide_image(binning, dtype):
    X, ref = _image(70, WIDE, dtype), _ref_sums(70, WIDE, dtype)
    cm = _check_sums(binning, X, WIDE, "cm", ref)
    pm = _check_sums(binning, X, WIDE, "pm", ref)
    bT, bA = _sum_bounds(70, WIDE, WIDE_BINS)
    assert abs(cm[0] - pm[0]) <= bT * cm[0] and abs(cm[1] - pm[1]) <= bT * cm[1]
    assert (np.abs(cm[2] - pm[2]) <= bA * cm[2]).all() and (np.abs(cm[3] - pm[3]) <= bA * cm[3]).all()


@pytest.mark.parametrize("layout,dtype", [("cm", "float32"), ("pm", "uint8")])
def test_binning_sums_read_no_padding(binning, layout, dtype):
    _check_sums(binning, _image(70, (37, 67), dtype), (37, 67), layout, _ref_sums(70, (37, 67), dtype), padded=True)


def test_risk_and_default_bins(binning):
    X = _image(70, (16, 24), "uint8")
    bins, var, bias, risk = binning.binning_risk(X, (16, 24))
    assert bins == [(b, b) for b in range(1, 9)]
    rv, rb, rr = br.risk(*br.sums(X, (16, 24), bins), 70, (16, 24))
    assert np.allclose(var, rv, rtol=1e-12, atol=0) and np.allclose(risk, rr, rtol=1e-9, atol=0)
    assert np.allclose(bias, rb, rtol=0, atol=1e-9 * np.abs(rr).max())


def test_best_binning_finds_the_block_size(binning):
    """The truth is constant on 4 x 4 blocks: X = min(Poisson(20 W H), 255), W gamma(1, 1) (300, 3), H Dirichlet(0.3) per block, 16 x 24
    pixels, numpy.random.default_rng(0).  First the numpy reference's own minimum (at 4, the second-lowest risk at least twice the
    lowest), then the device's."""
    shape = (16, 24)
    X, _, _ = br.block_image(300, shape, 4, seed=0)
    bins = [(b, b) for b in range(1, 9)]
    rrisk = br.risk(*br.sums(X, shape, bins), 300, shape)[2]
    order = np.argsort(rrisk)
    print("reference risk", rrisk)
    assert bins[order[0]] == (4, 4) and rrisk[order[0]] > 0 and rrisk[order[1]] >= 2 * rrisk[order[0]]
    assert binning.estimate_best_binning(X, shape, bins=bins) == (4, 4)
    risk, best = binning.estimate_best_binning(np.ascontiguousarray(X.T), shape, inspect=True, layout="pm")   # the default candidates: 1..8
    assert best == (4, 4) and risk.shape == (8,) and int(np.argmin(risk)) == int(order[0])
    from espm_amd import hyperspy_adapter as ha
    sig = ha.SpectrumImage(np.ascontiguousarray(X.T).reshape(16, 24, 300))
    assert sig.estimate_best_binning() == (4, 4)
    small = sig.rebin((4, 4))
    assert isinstance(small, ha.SpectrumImage) and small.data.shape == (4, 6, 300)
    assert np.array_equal(small.X.astype(np.int64), br.rebin_exact(X, shape, (4, 4)))


# ---- fit_binned ------------------------------------------------------------------------------------------------------------------------
N, SHAPE, BIN, K = 70, (32, 48), (4, 4), 3
COARSE = (SHAPE[0] // BIN[0], SHAPE[1] // BIN[1])
B = BIN[0] * BIN[1]


@functools.lru_cache(maxsize=None)
def _counts():
    X = br.block_image(N, SHAPE, 4, k=K, seed=5)[0]
    X.setflags(write=False)
    return X


def _est(**kw):
    from espm_amd.estimators import SmoothNMF
    args = dict(n_components=K, lambda_L=1.0, max_iter=30, verbose=0, random_state=0, shape_2d=SHAPE)
    args.update(kw)
    return SmoothNMF(**args)


def _upsample(Hb):
    return np.asarray(Hb, dtype=np.float64).reshape(K, *COARSE).repeat(BIN[0], axis=1).repeat(BIN[1], axis=2).reshape(K, -1)


def _by_hand(X, **kw):
    """fit_binned with what existed before it: numpy binning, fit_transform on the binned image, the rescaling rules, unmix."""
    est = _est(**dict(kw, shape_2d=COARSE))
    Xb = br.rebin_exact(X, SHAPE, BIN).astype(np.float32)
    est.fit_transform(np.ascontiguousarray(Xb.T) if est.hspy_comp else Xb)
    Wb, Hb = est.W_, est.H_
    H0 = _upsample(Hb)
    if est.normalize:
        est.norm_factor_ = est.norm_factor_ * B
        est.W_ = est.W_ / B
    elif est.simplex_W:
        H0 = H0 / B
    else:
        est.W_ = est.W_ / B
    if est.simplex_H:
        H0 = H0 / H0.sum(axis=0, keepdims=True)
    est.shape_2d = SHAPE
    Xin = np.ascontiguousarray(X.T) if est.hspy_comp else X
    H = est.unmix(Xin, H=H0.T if est.hspy_comp else H0)
    return est, Wb, Hb, H0, H


VARIANTS = [dict(simplex_H=True, normalize=True), dict(simplex_H=False, normalize=False),
            dict(simplex_H=True, simplex_W=False, normalize=False)]


@pytest.mark.parametrize("kw", VARIANTS, ids=["simplexH_normalize", "simplexW_plain", "simplexH_only"])
def test_fit_binned_is_the_steps_done_by_hand(kw):
    X = _counts()
    est = _est(**kw)
    H = est.fit_binned(X, BIN)
    ref, Wb, Hb, H0, Href = _by_hand(X, **kw)
    assert est.bin_ == BIN and est.binned_shape_2d_ == COARSE and tuple(est.shape_2d) == SHAPE
    assert est.W_binned_.shape == (N, K) and est.H_binned_.shape == (K, COARSE[0] * COARSE[1]) and H.shape == (K, SHAPE[0] * SHAPE[1])
    assert np.array_equal(est.W_binned_, Wb) and np.array_equal(est.H_binned_, Hb)
    assert np.array_equal(est.W_, ref.W_) and np.array_equal(H, Href) and np.array_equal(est.H_, Href)
    assert est.n_iter_ == ref.n_iter_ and est.losses_ == ref.losses_
    assert est.transform_n_iter_ == ref.transform_n_iter_ >= 1 and est.transform_losses_ == ref.transform_losses_
    nf = 1.0
    if est.normalize:
        assert est.norm_factor_ == ref.norm_factor_
        from espm_amd.estimators.base import normalization_factor
        assert np.isclose(est.norm_factor_, normalization_factor(np.asarray(X, dtype=np.float64), K), rtol=1e-6, atol=0)
        nf = est.norm_factor_
    # a pixel's model is its bin's model over B
    G = np.asarray(est.G_, dtype=np.float64)
    start = G @ (np.asarray(est.W_, dtype=np.float64) * nf) @ H0
    coarse = _upsample_model(G @ np.asarray(est.W_binned_, dtype=np.float64) @ np.asarray(est.H_binned_, dtype=np.float64)) / B * nf
    assert np.allclose(start, coarse, rtol=1e-6, atol=0)


def _upsample_model(Y):
    return Y.reshape(N, *COARSE).repeat(BIN[0], axis=1).repeat(BIN[1], axis=2).reshape(N, -1)


def test_fit_binned_through_the_adapter():
    from espm_amd import hyperspy_adapter as ha
    X = _counts()
    kw = dict(simplex_H=True, normalize=True, hspy_comp=True)
    sig = ha.SpectrumImage(np.ascontiguousarray(X.T).reshape(*SHAPE, N))
    est = _est(**dict(kw, shape_2d=None))
    lr = ha.decompose(sig, est, bin=BIN)
    ref, Wb, Hb, H0, Href = _by_hand(X, **kw)
    assert lr.decomposition_algorithm is est and tuple(est.shape_2d) == SHAPE
    assert lr.loadings.shape == (SHAPE[0] * SHAPE[1], K) and lr.factors.shape == (N, K)
    assert sig.get_decomposition_loadings().shape == (K, *SHAPE)
    assert np.array_equal(est.W_binned_, Wb) and np.array_equal(est.W_, ref.W_) and np.array_equal(lr.loadings, Href)
    assert np.array_equal(est.H_, Href.T) and np.array_equal(lr.factors, (est.G_ @ est.W_))


def test_a_plain_fit_after_fit_binned_is_a_fresh_fit():
    X = np.asarray(_counts(), dtype=np.float32)
    kw = dict(simplex_H=True, normalize=True)
    est = _est(**kw)
    est.fit_binned(X, BIN)
    assert tuple(est.shape_2d) == SHAPE
    for diag in (est.pixel_diagnostics, est.spectral_diagnostics):   # X_ is the binned image: the full-resolution X is asked for
        with pytest.raises(ValueError, match="fit_binned"):
            diag()
    assert est.pixel_diagnostics(X)["deviance"].shape == (SHAPE[0] * SHAPE[1],)
    est.fit(X)
    assert not any(hasattr(est, name) for name in ("bin_", "binned_shape_2d_", "W_binned_", "H_binned_"))
    assert est.pixel_diagnostics()["deviance"].shape == (SHAPE[0] * SHAPE[1],)
    fresh = _est(**kw).fit(X)
    for name in ("W_", "H_", "components_", "X_"):
        assert np.array_equal(getattr(est, name), getattr(fresh, name)), name
    assert est.n_iter_ == fresh.n_iter_ and est.losses_ == fresh.losses_ and est.norm_factor_ == fresh.norm_factor_
    assert est.reconstruction_err_ == fresh.reconstruction_err_ and est.L_.shape == fresh.L_.shape
