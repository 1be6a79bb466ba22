"""Count attribution without a device: the rule and the expected attribution in numpy (tests/attribution_reference.py) and their
properties, ``get_explained_intensity_W`` against the reference's stored results, the binding, the argument checks of the entry points
that come before any launch, the wide builds' stubs, and what the module and the estimator refuse before anything is uploaded."""
import ctypes as C
import os

import numpy as np
import pytest

from abi_header import CTYPE, _declared
import attribution_reference as ar
import splitting_reference as sr

N, P = 96, 1320
SEEDS = [0, (1 << 40) + 3]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f22_explained_intensity.npz")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def split():
    """The 16-bit test image, the planted model at k = 3 and its reference attribution under both seeds."""
    X = sr.image()
    D, H = ar.planted_model(N, P, 3)
    return X, D, H, {seed: ar.assign(X, D, H, seed) for seed in SEEDS}


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
def test_the_parts_add_up_and_the_invalid_entries_are_the_planted_ones(split):
    X, D, H, got = split
    planted = np.zeros(X.shape, dtype=bool)
    planted[20, :] = planted[:, 500] = planted[:, 11] = True   # the zero row of D, the zero columns of H
    for seed in SEEDS:
        parts, invalid = got[seed]
        assert parts.dtype == X.dtype and parts.shape == (3,) + X.shape
        assert np.array_equal(parts.astype(np.int64).sum(axis=0), X)
        assert invalid == int((planted & (X > 0)).sum()) > 0
        assert np.array_equal(parts[0][planted], X[planted]) and not parts[1:][:, planted].any()
    assert not np.array_equal(got[SEEDS[0]][0], got[SEEDS[1]][0])
    assert np.array_equal(ar.assign(X, D, H, SEEDS[0])[0], got[SEEDS[0]][0])
    # every component gets its share of the largest entry: 65535 counts at rates s_0, s_1 - s_0, s_2 - s_1
    S = ar.rates(D, H)[:, 48, 660]
    share = np.diff(np.concatenate([[0.0], S])) / S[-1]
    sigma = np.sqrt(65535 * share * (1 - share))
    assert (np.abs(got[0][0][:, 48, 660] - 65535 * share) < 5 * sigma).all()


def test_one_component_keeps_the_image():
    X = sr.image()
    D, H = sr.model(N, P, 1)
    parts, invalid = ar.assign(X, D, H, 9)
    assert invalid == int((X[:, 11] > 0).sum())   # (the model's own zero column)
    assert np.array_equal(parts[0], X)


def test_the_rule_is_invariant_under_slabs_and_layout(split):
    X, D, H, got = split
    seed = SEEDS[1]
    whole = got[seed][0]
    # a slab of pixels attributed alone is that slab of the whole
    slab, _ = ar.assign(X[:, 500:820], D, H[:, 500:820], seed, p_total=P, j0=500)
    assert np.array_equal(slab, whole[:, :, 500:820])
    assert not np.array_equal(ar.assign(X[:, 500:820], D, H[:, 500:820], seed)[0], slab)   # without the geometry: another split
    # the index is the logical (channel, pixel) one: a pixel-major copy of the image is attributed as its transpose
    assert np.array_equal(ar.assign(np.ascontiguousarray(X.T).T, D, H, seed)[0], whole)
    # the last 700 pixels of an image of 2^31 pixels: the indices of channels 2 and 3 are past 2^32
    p_total, p = 1 << 31, 700
    Xs = np.ascontiguousarray(X[44:48, 600:1300])
    Ds, Hs = sr.model(4, p, 5)
    far, _ = ar.assign(Xs, Ds, Hs, seed, p_total=p_total, j0=p_total - p)
    assert np.array_equal(far.astype(np.int64).sum(axis=0), Xs)
    assert 3 * p_total + (p_total - p) > 1 << 32 and not np.array_equal(far, ar.assign(Xs, Ds, Hs, seed)[0])
    assert np.array_equal(far[:, :, 100:400], ar.assign(Xs[:, 100:400], Ds, Hs[:, 100:400], seed, p_total=p_total, j0=p_total - p + 100)[0])


def test_the_counters_are_neither_thinning_s_nor_sampling_s():
    """Word sets of a few elements under one seed: thinning has (e, d div 4 < 2^14, 0), sampling (e, block, replicate + 1 >= 1), the
    attribution (e, 2^31 | d div 4, 0)."""
    seed = (1 << 40) + 3
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for e, x in ((0, 1), (7, 300), (96 * 1320 - 1, 65535), ((1 << 33) + 5, 65535)):
        mine = ar.words(e, x, seed)
        assert len(mine) == (x + 3) // 4 and all(c[2] >= 1 << 31 and c[3] == 0 for c, _ in mine)
        thinning = {((e & 0xFFFFFFFF, e >> 32, b, 0), key) for b in range((x + 3) // 4)}
        sampling = {((e & 0xFFFFFFFF, e >> 32, b, r + 1), key) for b in range(4 + (65535 + 3) // 4) for r in (0, 1, 2 ** 32 - 2)}
        assert max(c[2] for c, _ in thinning) < 1 << 14
        assert not mine & thinning and not mine & sampling
    # and the words themselves differ: the first block of element 7
    mine = sr.philox4x32((7, 0, ar.MARK, 0), key)
    assert [int(w) for w in mine] != [int(w) for w in sr.philox4x32((7, 0, 0, 0), key)]


def test_the_totals_are_multinomial(split):
    """The per-component totals against their multinomial expectation, |z| < 4.5: a condition on the rule and the committed seeds.
    The reference sits at z = +0.47, -1.59, +1.17 (seed 0) and -0.53, -0.20, +0.81 (seed 2^40 + 3) on the 16-bit image."""
    X, D, H, got = split
    for seed in SEEDS:
        z = ar.multinomial_z(X, D, H, got[seed][0])
        print(f"seed {seed}: z = " + ", ".join(f"{v:+.2f}" for v in z))
        assert (np.abs(z) < 4.5).all()
    # entry by entry: over the valid entries with one count, the fraction that goes to component i is the mean of its probability
    S = ar.rates(D, H)
    one = (X == 1) & (S[-1] > 0)
    for i in range(3):
        pr = ((S[i] - (S[i - 1] if i else 0.0)) / np.where(S[-1] > 0, S[-1], 1.0))[one]
        assert abs(got[0][0][i][one].mean() - pr.mean()) < 5 * np.sqrt((pr * (1 - pr)).sum()) / one.sum()


# ---- the expected attribution ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint16", "float64"])
def test_reference_expected_identities(dtype):
    X = sr.image().astype(dtype)
    D, H = ar.planted_model(N, P, 3)
    ref = ar.expected(X, D, H)
    assert ref["counts"].dtype == (np.int64 if dtype == "uint16" else np.float64) and np.array_equal(ref["counts"], X.sum(axis=0))
    y_ok = (D @ H >= ar.LOG_SHIFT).all(axis=0) | (X[20] == 0)   # pixels whose every non-zero entry has a model
    y_ok[[11, 500]] = False
    assert y_ok.sum() > 500
    assert (np.abs(ref["unattributed"])[y_ok] <= ref["identity_bound"][y_ok]).all()
    assert ref["unattributed"][500] == X[:, 500].sum() and ref["unattributed"][11] == X[:, 11].sum()
    left = X[20].astype(np.float64)
    left[[11, 500]] = X[:, [11, 500]].sum(axis=0)
    assert (np.abs(ref["unattributed"] - left) <= ref["identity_bound"]).all()
    assert (np.abs(ref["channel_counts"].sum(axis=0) - ref["pixel_counts"].sum(axis=1)) <= ref["totals_bound"]).all()
    assert (ref["pixel_bound"] >= 0).all() and (ref["pixel_bound"] <= 1e-12 * np.maximum(ref["pixel_counts"], 1e-300)).all()
    assert ar.gamma(1) == ar.U / (1 - ar.U)


def test_intensity_is_w_times_gt_r(lib):
    from espm_amd import attribution
    rng = np.random.default_rng(0)
    G, W, R = rng.random((9, 4)), rng.random((4, 3)), rng.random((9, 3))
    want = np.array([[W[i, j] * sum(G[c, i] * R[c, j] for c in range(9)) for j in range(3)] for i in range(4)])
    np.testing.assert_allclose(attribution.intensity(G, W, R), want, rtol=1e-14)
    D = rng.random((9, 3))
    assert np.array_equal(attribution.intensity(None, D, R), D * R)
    with pytest.raises(ValueError):
        attribution.intensity(G, W, R[:8])
    with pytest.raises(ValueError):
        attribution.intensity(None, W, R)


def test_explained_intensity_against_the_triple_loop_and_the_reference(lib):
    from espm_amd.utils import get_explained_intensity_W
    rng = np.random.default_rng(1)
    G, W, H = rng.random((10, 4)), rng.random((4, 3)), rng.random((3, 12))
    loop = np.zeros(W.shape)
    for i in range(4):
        for j in range(3):
            loop[i, j] = sum(G[c, i] * W[i, j] * H[j, q] for c in range(10) for q in range(12))
    np.testing.assert_allclose(get_explained_intensity_W(G, W, H), loop, rtol=1e-13)
    with np.load(GOLDEN) as z:
        for name in ("dict", "one", "eye"):
            got = get_explained_intensity_W(z[name + "_G"], z[name + "_W"], z[name + "_H"])
            assert got.shape == z[name + "_W"].shape and np.array_equal(got, z[name + "_out"]), name
        assert z["dict_out"][1, 0] == 0.0


# ---- the binding ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["espm_attribute_expected", "espm_attribute_expected_scratch", "espm_assign_counts"])
def test_symbols_are_bound_with_the_headers_signatures(lib, name):
    res, args = lib.SYMBOLS[name]
    cres, cargs = _declared(name)
    assert res is CTYPE[cres]
    assert list(args) == [CTYPE[a] for a in cargs]
    for handle in (lib.lib, lib.variant(12).lib, lib.variant(20).lib):
        assert hasattr(handle, name)


def test_header_and_packaged_copy_carry_the_sizes(lib):
    from espm_amd import _abi, attribution
    d = _abi.parse_defines(_abi.header_text())
    assert d["ESPM_ATTRIB_BLOCK"] == lib.ATTRIB_BLOCK == 256 and d["ESPM_ATTRIB_HEAVY"] == lib.ATTRIB_HEAVY == 256
    assert d["ESPM_ATTRIB_PCHUNK"] == lib.ATTRIB_PCHUNK == ar.PCHUNK and d["ESPM_ATTRIB_WALK"] == lib.ATTRIB_WALK == 512
    assert d["ESPM_ATTRIB_MAX_K"] == lib.ATTRIB_MAX_K == attribution.MAX_K == 32
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert open(os.path.join(root, "include", "espm_mu.h")).read() == open(os.path.join(root, "espm_amd", "include", "espm_mu.h")).read()


U8, U16, F32, F64, CM, PM = 0, 1, 2, 3, 0, 1


def _vp(v):
    return None if v is None else C.c_void_p(v)   # (never dereferenced: every call below is refused on the host)


def _expected(f, x=8, dtype=U8, layout=CM, ld=80, n=8, p=80, d=8, h=8, k=3, log_shift=1e-14, num=8, ratio=8, counts=8, scratch=8,
              scratch_bytes=1 << 20):
    return f(_vp(x), dtype, layout, ld, n, p, _vp(d), _vp(h), k, log_shift, _vp(num), _vp(ratio), _vp(counts), _vp(scratch), scratch_bytes, None)


def test_expected_argument_errors_need_no_device(lib):
    f, err = lib.lib.espm_attribute_expected, lib.lib.espm_mu_last_error
    names = ("x", "d", "h", "num", "ratio", "counts", "scratch")
    assert _expected(f, **{name: None for name in names}) == lib.EINVAL      # the null call
    for name in names:
        assert _expected(f, **{name: None}) == lib.EINVAL, name
    assert _expected(f, k=0) == lib.EINVAL and b"k=0" in err()
    assert _expected(f, k=33) == lib.EINVAL and b"k=33" in err()
    assert _expected(f, n=0) == lib.EINVAL and b"n=0" in err()
    assert _expected(f, p=0) == lib.EINVAL and b"p=0" in err()
    assert _expected(f, dtype=4) == lib.EINVAL and b"x_dtype 4" in err()
    assert _expected(f, dtype=-1) == lib.EINVAL
    assert _expected(f, layout=2) == lib.EINVAL and b"x_layout 2" in err()
    assert _expected(f, ld=79) == lib.EINVAL and b"ld=79" in err()
    assert _expected(f, layout=PM, ld=7) == lib.EINVAL and b"ld=7" in err()      # pixel-major: rows of n
    assert _expected(f, log_shift=0.0) == lib.EINVAL and b"log_shift=0" in err()
    assert _expected(f, log_shift=-1.0) == lib.EINVAL and _expected(f, log_shift=float("nan")) == lib.EINVAL
    # the scratch: chunks x k x n doubles, chunks of ESPM_ATTRIB_PCHUNK pixels
    q = lib.lib.espm_attribute_expected_scratch
    assert q(8, 80, 3) == 1 * 3 * 8 * 8 and q(96, 1320, 5) == 2 * 5 * 96 * 8 and q(2048, 512 * 512, 5) == 256 * 5 * 2048 * 8
    assert q(0, 80, 3) == q(8, 0, 3) == q(8, 80, 0) == q(8, 80, 33) == 0
    assert _expected(f, scratch_bytes=q(8, 80, 3) - 1) == lib.EINVAL and b"191 bytes, 192 needed" in err()
    with pytest.raises(ValueError):
        lib.check(lib.EINVAL)


def _assign(f, x=8, dtype=U8, layout=CM, ld=80, n=8, p=80, p_total=80, j0=0, d=8, h=8, k=3, seed=0, parts=8, part_stride=640, out_ld=80, counts=8):
    return f(_vp(x), dtype, layout, ld, n, p, p_total, j0, _vp(d), _vp(h), k, seed, _vp(parts), part_stride, out_ld, _vp(counts), None)


def test_assign_argument_errors_need_no_device(lib):
    f, err = lib.lib.espm_assign_counts, lib.lib.espm_mu_last_error
    names = ("x", "d", "h", "parts", "counts")
    assert _assign(f, **{name: None for name in names}) == lib.EINVAL      # the null call
    for name in names:
        assert _assign(f, **{name: None}) == lib.EINVAL, name
    assert _assign(f, k=0) == lib.EINVAL and b"k=0" in err()
    assert _assign(f, k=33) == lib.EINVAL and b"k=33" in err()
    assert _assign(f, n=0) == lib.EINVAL and b"n=0" in err()
    assert _assign(f, p=0, p_total=0) == lib.EINVAL and b"p=0" in err()
    assert _assign(f, dtype=F32) == lib.EINVAL and b"x_dtype 2" in err()       # counts only
    assert _assign(f, dtype=F64) == lib.EINVAL and _assign(f, dtype=-1) == lib.EINVAL
    assert _assign(f, layout=2) == lib.EINVAL and b"x_layout 2" in err()
    assert _assign(f, ld=79) == lib.EINVAL and b"ld=79" in err()
    assert _assign(f, layout=PM, ld=7, out_ld=8) == lib.EINVAL and b"ld=7" in err()      # pixel-major: rows of n
    assert _assign(f, out_ld=79) == lib.EINVAL and b"out_ld=79" in err()
    assert _assign(f, layout=PM, ld=8, out_ld=7) == lib.EINVAL and b"out_ld=7" in err()
    assert _assign(f, part_stride=639) == lib.EINVAL and b"part_stride=639" in err()     # the images would overlap
    assert _assign(f, out_ld=90, part_stride=7 * 90 + 79) == lib.EINVAL and b"part_stride=709" in err()   # (padded rows: 7 x 90 + 80)
    assert _assign(f, p_total=79) == lib.EINVAL and b"p_total=79" in err()                # the image is smaller than its slab
    assert _assign(f, p_total=100, j0=21) == lib.EINVAL and b"j0=21" in err()             # the slab ends behind the image
    assert _assign(f, p_total=100, j0=-1) == lib.EINVAL and b"j0=-1" in err()
    assert _assign(f, p_total=1 << 62) == lib.EINVAL and b"64-bit" in err()               # n x p_total overflows the index


def test_the_wide_builds_export_stubs(lib):
    for k in (12, 20):
        v = lib.variant(k)
        rc = v.lib.espm_attribute_expected(None, 0, 0, 8, 8, 8, None, None, k, 1e-14, None, None, None, None, 0, None)
        assert rc == lib.EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            v.check(rc)
        assert v.lib.espm_attribute_expected_scratch(8, 8, k) == 0
        assert v.lib.espm_assign_counts(None, 0, 0, 8, 8, 8, 8, 0, None, None, k, 0, None, 64, 8, None, None) == lib.EUNSUPPORTED


# ---- the Python module and the estimator, before the device ---------------------------------------------------------------------------------
def test_module_raises_before_upload(lib, monkeypatch):
    import torch

    from espm_amd import attribution
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X = np.zeros((6, 20), np.uint8)
    D, H = np.ones((6, 2)), np.ones((2, 20))
    with pytest.raises(TypeError, match="defined for counts"):
        attribution.assign(X.astype(np.float32), D, H)
    with pytest.raises(TypeError, match="defined for counts"):
        attribution.assign(torch.zeros((6, 20), dtype=torch.float64), D, H)
    big = X.astype(np.int64)
    big[2, 3] = 65536
    with pytest.raises(ValueError, match="to 65536"):
        attribution.assign(big, D, H)
    neg = X.astype(np.int32)
    neg[2, 3] = -1
    with pytest.raises(ValueError, match="from -1 to 0"):
        attribution.assign(neg, D, H)
    for seed in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            attribution.assign(X, D, H, seed=seed)
    for call in (attribution.assign, attribution.expected):
        with pytest.raises(ValueError, match="layout"):
            call(X, D, H, layout="rows")
        with pytest.raises(ValueError, match="2-D"):
            call(np.zeros(6, np.uint8), D, H)
        with pytest.raises(ValueError, match="channels"):
            call(X, np.ones((5, 2)), H)
        with pytest.raises(ValueError, match="pixels"):
            call(X, D, np.ones((2, 19)))
        with pytest.raises(ValueError, match="X has 20 channels"):   # (pixel-major: the 6 x 20 array is 6 pixels of 20 channels)
            call(X, D, H, layout="pm")
        with pytest.raises(ValueError, match="components"):
            call(X, np.ones((6, 2)), np.ones((3, 20)))
        with pytest.raises(NotImplementedError, match="33 components"):
            call(X, np.ones((6, 33)), np.ones((33, 20)))
    with pytest.raises(ValueError, match="log_shift"):
        attribution.expected(X, D, H, log_shift=0)
    with pytest.raises(ValueError, match="log_shift"):
        attribution.expected(X.astype(np.float32), D, H, log_shift=-1.0)


def test_no_cpu_fallback(lib, monkeypatch):
    import torch

    from espm_amd import attribution
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X = np.zeros((6, 20), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        attribution.assign(X, np.ones((6, 2)), np.ones((2, 20)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        attribution.expected(X, np.ones((6, 2)), np.ones((2, 20)))


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


def test_estimator_refuses_before_any_upload(lib, monkeypatch):
    from sklearn.exceptions import NotFittedError

    from espm_amd import attribution
    from espm_amd.estimators import SmoothNMF
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X = np.ones((6, 20), np.uint8)
    with pytest.raises(NotFittedError):
        SmoothNMF(n_components=3, verbose=0).attribute_counts(X)
    with pytest.raises(NotFittedError):
        SmoothNMF(n_components=3, verbose=0).assign_counts(X)
    # attribute_counts: X as for pixel_diagnostics
    with pytest.raises(ValueError, match="X has 5 channels"):
        _fitted().attribute_counts(X[:5])
    with pytest.raises(ValueError, match="X has 19 pixels"):
        _fitted().attribute_counts(X[:, :19])
    with pytest.raises(ValueError, match="X has 20 channels"):
        _fitted(hspy_comp=True).attribute_counts(X)
    with pytest.raises(NotImplementedError, match="33 components"):
        _fitted(n_components=33).attribute_counts(X)
    binned = _fitted()
    binned.bin_ = (2, 2)
    with pytest.raises(ValueError, match="fit_binned"):
        binned.attribute_counts()
    # assign_counts: X is required, counts only, one GPU, no binned fit
    with pytest.raises(TypeError):
        _fitted().assign_counts()
    with pytest.raises(NotImplementedError, match="assign_counts does not cover shard"):
        _fitted().shard(object()).assign_counts(X)
    with pytest.raises(ValueError, match="fit_binned"):
        binned.assign_counts(X)
    with pytest.raises(TypeError, match="defined for counts"):
        _fitted().assign_counts(X.astype(np.float32))
    with pytest.raises(ValueError, match="X has 5 channels"):
        _fitted().assign_counts(X[:5])
    with pytest.raises(ValueError, match="seed"):
        _fitted().assign_counts(X, seed=-1)
    with pytest.raises(NotImplementedError, match="33 components"):
        _fitted(n_components=33).assign_counts(X)
    for name in ("pixel_counts_", "channel_counts_", "intensity_W_"):
        assert not hasattr(binned, name)


def test_adapter_needs_the_attribution_first(lib):
    from espm_amd import hyperspy_adapter as ha
    est = _fitted()
    with pytest.raises(AttributeError, match="attribute_counts"):
        ha.component_count_maps(est)
    with pytest.raises(AttributeError, match="attribute_counts"):
        ha.component_spectra(est)
    est.pixel_counts_, est.channel_counts_ = np.arange(60.0).reshape(3, 20), np.arange(18.0).reshape(6, 3)
    assert ha.component_count_maps(est).shape == (3, 4, 5) and ha.component_count_maps(est, shape_2d=(2, 10)).shape == (3, 2, 10)
    assert np.array_equal(ha.component_spectra(est), est.channel_counts_.T)

    class Est:
        hspy_comp = True

        def assign_counts(self, X, seed=0):
            self.seen = (X.shape, seed)
            return np.stack([X, np.zeros_like(X)])

    sig, e = ha.SpectrumImage(np.arange(8 * 12 * 7).reshape(8, 12, 7).astype(np.uint16)), Est()
    images = sig.assign_counts(e, seed=4)
    assert e.seen == ((96, 7), 4) and len(images) == 2 and np.array_equal(images[0].data, sig.data) and not images[1].data.any()
    e.hspy_comp = False
    images = sig.assign_counts(e, seed=4)
    assert e.seen == ((7, 96), 4) and np.array_equal(images[0].data, sig.data)
