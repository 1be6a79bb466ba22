"""Count splitting without a device: Philox4x32-10 and the thinning rule in numpy (tests/splitting_reference.py), the binding, the
argument checks of the entry points that come before any launch, the wide builds' stubs, and what ``thin`` and ``fit_split`` refuse
before anything is uploaded."""
import ctypes as C

import numpy as np
import pytest

from abi_header import CTYPE, _declared
import splitting_reference as sr


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


# ---- the reference itself -------------------------------------------------------------------------------------------------------
def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    """The known-answer vectors of Random123 (kat_vectors, philox4x32 with 10 rounds)."""
    assert _hex(sr.philox4x32((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(sr.philox4x32((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert (_hex(sr.philox4x32((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)))
            == "d16cfe09 94fdcceb 5001e420 24126ea1")
    # arrays go through word by word
    w = sr.philox4x32((np.array([0, 0xFFFFFFFF], dtype=np.uint64), np.array([0, 0xFFFFFFFF], dtype=np.uint64),
                       np.array([0, 0xFFFFFFFF], dtype=np.uint64), np.array([0, 0xFFFFFFFF], dtype=np.uint64)), (0, 0))
    assert int(w[0][0]) == 0x6627E8D5 and w[0].dtype == np.uint32


def test_threshold():
    assert sr.threshold(0.5) == (1 << 31, 0.5)
    assert sr.threshold(0.8)[0] == round(0.8 * 2 ** 32) == 3435973837
    assert sr.threshold(2.0 ** -40) == (1, 2.0 ** -32) and sr.threshold(1 - 2.0 ** -40) == (2 ** 32 - 1, 1 - 2.0 ** -32)


def _small(seed=12345):
    return np.random.default_rng(seed).poisson(0.6, size=(96, 1320)).astype(np.uint16)


def test_reference_split_adds_up_and_keeps_planted_entries():
    X = sr.image()
    for q in (0.5, 0.8):
        Xa, Xb = sr.thin(X, sr.threshold(q)[0], 7)
        assert Xa.dtype == X.dtype and np.array_equal(Xa.astype(np.int64) + Xb, X)
    assert X[48, 660] == 65535 and X[3, 64] == 256 and X[17, 700] == 300 and X[0, 0] == 1 and X[5, 7] == 255
    # a 65535 at q = 0.8: 52428 expected, sigma 102
    assert abs(int(Xa[48, 660]) - 0.8 * 65535) < 5 * 103
    # the extremes: thr = 1 sends (almost surely) nothing to A, thr = 2^32 - 1 everything
    Xa, Xb = sr.thin(X, 1, 0)
    assert Xa.sum() == 0 and np.array_equal(Xb, X)
    Xa, Xb = sr.thin(X, 2 ** 32 - 1, 0)
    assert np.array_equal(Xa, X) and Xb.sum() == 0


def test_reference_split_is_invariant_under_layout_and_slabs():
    X = _small()
    thr = sr.threshold(0.8)[0]
    seed = (1 << 40) + 3
    Xa, Xb = sr.thin(X, thr, seed)
    # a slab of pixels split alone is that slab of the whole split
    Sa, Sb = sr.thin(X[:, 500:820], thr, seed, p_total=1320, j0=500)
    assert np.array_equal(Sa, Xa[:, 500:820]) and np.array_equal(Sb, Xb[:, 500:820])
    # the index is the logical (channel, pixel) one: a pixel-major copy of the image is split as its transpose
    Ta, _ = sr.thin(np.ascontiguousarray(X.T).T, thr, seed)
    assert np.array_equal(Ta, Xa)
    # without the geometry the slab is another split
    assert not np.array_equal(sr.thin(X[:, 500:820], thr, seed)[0], Sa)


def test_reference_split_differs_between_seeds():
    X = _small()
    thr = sr.threshold(0.5)[0]
    A0, A1, A2 = (sr.thin(X, thr, s)[0] for s in (0, 1, 1 << 32))
    assert not np.array_equal(A0, A1) and not np.array_equal(A0, A2) and not np.array_equal(A1, A2)
    assert np.array_equal(A0, sr.thin(X, thr, 0)[0])


@pytest.mark.parametrize("q", [0.5, 0.8])
def test_reference_split_total_is_binomial(q):
    """The total of X_a is Binomial(N, q_eff): within 5 sigma of q N.  (This image - numpy's default_rng(12345).poisson(0.6), seed
    12345 - sits at +1.36 sigma for q = 0.5 and +0.16 sigma for q = 0.8.)"""
    X = _small()
    thr, q_eff = sr.threshold(q)
    Xa, _ = sr.thin(X, thr, 12345)
    N = float(X.sum())
    z = (float(Xa.sum()) - q_eff * N) / np.sqrt(N * q_eff * (1 - q_eff))
    print(f"q = {q}: total of X_a at {z:+.2f} sigma")
    assert abs(z) < 5
    # and entry by entry: the mean of x_a over the entries with x = 1, 2, 3 is q x
    for v in (1, 2, 3):
        m = X == v
        assert abs(Xa[m].mean() - q_eff * v) < 5 * np.sqrt(v * q_eff * (1 - q_eff) / m.sum())


def test_reference_deviances():
    """The held-out deviance of the materialised X_b against r Y; zero counts add their y; the bound is positive and small."""
    X = sr.image(dtype=np.uint8)[:, :200]
    thr, q_eff = sr.threshold(0.8)
    Xa, Xb = sr.thin(X, thr, 0)
    D, H = sr.model(96, 200, 3)
    ref = sr.deviances(Xa, Xb, D, H, thr)
    Y = np.maximum(D @ H, sr.LOG_SHIFT)
    r = (1 - q_eff) / q_eff
    j = 5
    xb = Xb[:, j].astype(float)
    t = np.where(xb > 0, xb * np.log(np.where(xb > 0, xb, 1) / (r * Y[:, j])), 0.0) - xb + r * Y[:, j]
    assert abs(ref["heldout_map"][j] - 2 * t.sum()) <= 1e-12 * abs(2 * t.sum())
    assert ref["heldout_counts"].dtype == np.int64 and ref["heldout_counts"].sum() == Xb.sum()
    assert np.isfinite(ref["train_map"]).all() and np.isfinite(ref["heldout_map"]).all()   # (pixel 11 is at the log_shift floor)
    assert (ref["train_bound"] > 0).all() and (ref["train_bound"] < 1e-9 * np.maximum(ref["train_map"], 1)).all()


# ---- the binding ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["espm_thin_counts", "espm_split_deviance"])
def test_symbols_are_bound_with_the_headers_signatures(lib, name):
    res, args = lib.SYMBOLS[name]
    cres, cargs = _declared(name)
    assert res is CTYPE[cres]
    assert list(args) == [CTYPE[a] for a in cargs]
    assert hasattr(lib.lib, name)


def test_header_and_packaged_copy_carry_the_sizes(lib):
    import os

    from espm_amd import _abi
    d = _abi.parse_defines(_abi.header_text())
    assert d["ESPM_SPLIT_BLOCK"] == lib.SPLIT_BLOCK == 256 and d["ESPM_SPLIT_HEAVY"] == lib.SPLIT_HEAVY == 256
    assert d["ESPM_SPLIT_MAX_K"] == lib.SPLIT_MAX_K == 32
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert open(os.path.join(root, "include", "espm_mu.h")).read() == open(os.path.join(root, "espm_amd", "include", "espm_mu.h")).read()


U8, U16, CM, PM = 0, 1, 0, 1
HALF = 1 << 31


def _thin(f, x=8, dtype=U8, layout=CM, ld=80, n=8, p=80, p_total=80, j0=0, thr=HALF, seed=0, xa=8, xb=8, out_ld=80):
    vp = lambda v: None if v is None else C.c_void_p(v)   # (never dereferenced: every call below is refused on the host)
    return f(vp(x), dtype, layout, ld, n, p, p_total, j0, thr, seed, vp(xa), vp(xb), out_ld, None)


def test_thin_argument_errors_need_no_device(lib):
    f, err = lib.lib.espm_thin_counts, lib.lib.espm_mu_last_error
    assert _thin(f, x=None, xa=None, xb=None) == lib.EINVAL      # the null call
    assert _thin(f, x=None) == lib.EINVAL
    assert _thin(f, xa=None) == lib.EINVAL
    assert _thin(f, n=0) == lib.EINVAL and b"n=0" in err()
    assert _thin(f, p=0, p_total=0) == lib.EINVAL and b"p=0" in err()
    assert _thin(f, dtype=lib.DIAG_X_F32) == lib.EINVAL and b"x_dtype 2" in err()       # counts only
    assert _thin(f, dtype=lib.DIAG_X_F64) == lib.EINVAL and _thin(f, dtype=-1) == lib.EINVAL
    assert _thin(f, layout=2) == lib.EINVAL and b"x_layout 2" in err()
    assert _thin(f, ld=79) == lib.EINVAL and b"ld=79" in err()
    assert _thin(f, layout=PM, ld=7, out_ld=8) == lib.EINVAL and b"ld=7" in err()      # pixel-major: rows of n
    assert _thin(f, out_ld=79) == lib.EINVAL and b"out_ld=79" in err()
    assert _thin(f, layout=PM, ld=8, out_ld=7) == lib.EINVAL and b"out_ld=7" in err()
    assert _thin(f, p_total=79) == lib.EINVAL and b"p_total=79" in err()                # the image is smaller than its slab
    assert _thin(f, p_total=100, j0=21) == lib.EINVAL and b"j0=21" in err()             # the slab ends behind the image
    assert _thin(f, p_total=100, j0=-1) == lib.EINVAL and b"j0=-1" in err()
    assert _thin(f, p_total=1 << 62) == lib.EINVAL and b"64-bit" in err()               # n x p_total overflows the index
    assert _thin(f, thr=0) == lib.EINVAL and b"q_threshold=0" in err()
    assert _thin(f, thr=1 << 32) == lib.EINVAL and b"q_threshold=4294967296" in err()
    assert _thin(f, thr=-5) == lib.EINVAL and b"q_threshold=-5" in err()
    with pytest.raises(ValueError):
        lib.check(lib.EINVAL)


def _dev(f, x=8, dtype=U8, layout=CM, ld=80, n=8, p=80, p_total=80, j0=0, thr=HALF, seed=0, d=8, h=8, k=3, log_shift=1e-14, da=8, db=8, cb=8):
    vp = lambda v: None if v is None else C.c_void_p(v)
    return f(vp(x), dtype, layout, ld, n, p, p_total, j0, thr, seed, vp(d), vp(h), k, log_shift, vp(da), vp(db), vp(cb), None)


def test_split_deviance_argument_errors_need_no_device(lib):
    f, err = lib.lib.espm_split_deviance, lib.lib.espm_mu_last_error
    assert _dev(f, x=None, d=None, h=None, da=None, db=None, cb=None) == lib.EINVAL     # the null call
    for name in ("x", "d", "h", "da", "db", "cb"):
        assert _dev(f, **{name: None}) == lib.EINVAL
    assert _dev(f, k=0) == lib.EINVAL and b"k=0" in err()
    assert _dev(f, k=33) == lib.EINVAL and b"k=33" in err()
    assert _dev(f, log_shift=0.0) == lib.EINVAL and b"log_shift=0" in err()
    assert _dev(f, log_shift=-1.0) == lib.EINVAL
    assert _dev(f, dtype=lib.DIAG_X_F32) == lib.EINVAL and b"x_dtype 2" in err()
    assert _dev(f, layout=-1) == lib.EINVAL
    assert _dev(f, ld=79) == lib.EINVAL and b"ld=79" in err()
    assert _dev(f, n=0) == lib.EINVAL and _dev(f, p=0) == lib.EINVAL
    assert _dev(f, p_total=100, j0=21) == lib.EINVAL and b"j0=21" in err()
    assert _dev(f, thr=0) == lib.EINVAL and _dev(f, thr=1 << 32) == lib.EINVAL and b"q_threshold=4294967296" in err()


def test_the_wide_builds_export_stubs(lib):
    for k in (12, 20):
        v = lib.variant(k)
        rc = v.lib.espm_thin_counts(None, 0, 0, 8, 8, 8, 8, 0, HALF, 0, None, None, 8, None)
        assert rc == lib.EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            v.check(rc)
        assert v.lib.espm_split_deviance(None, 0, 0, 8, 8, 8, 8, 0, HALF, 0, None, None, k, 1e-14, None, None, None, None) == lib.EUNSUPPORTED


# ---- the Python module, before the device ------------------------------------------------------------------------------------------------
def test_module_threshold(lib):
    from espm_amd import splitting
    for q in (0.5, 0.8, 0.25, 1e-3, 2.0 ** -40, 1 - 2.0 ** -40):
        assert splitting.threshold(q) == sr.threshold(q)
    for bad in (0, 1, -0.1, 1.5, float("nan"), "half", None):
        with pytest.raises(ValueError):
            splitting.threshold(bad)


def test_thin_raises_before_upload(lib, monkeypatch):
    import torch

    from espm_amd import _image, splitting
    from espm_amd._image_args import counts_image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X = np.zeros((6, 20), np.uint8)
    with pytest.raises(TypeError, match="defined for counts"):
        splitting.thin(X.astype(np.float32))
    with pytest.raises(TypeError, match="defined for counts"):
        splitting.thin(torch.zeros((6, 20), dtype=torch.float64))
    with pytest.raises(TypeError, match="defined for counts"):
        splitting.split_deviance(X.astype(np.float64), np.ones((6, 2)), np.ones((2, 20)))
    neg = X.astype(np.int32)
    neg[2, 3] = -1
    with pytest.raises(ValueError, match="from -1 to 0"):
        splitting.thin(neg)
    big = X.astype(np.int64)
    big[2, 3] = 65536
    with pytest.raises(ValueError, match="to 65536"):
        splitting.thin(big)
    with pytest.raises(ValueError, match="to 65536"):
        splitting.thin(torch.from_numpy(big))
    with pytest.raises(ValueError, match="layout"):
        splitting.thin(X, layout="rows")
    with pytest.raises(ValueError, match="2-D"):
        splitting.thin(np.zeros(6, np.uint8))
    for q in (0.0, 1.0, -1, 2):
        with pytest.raises(ValueError, match="between 0 and 1"):
            splitting.thin(X, q=q)
    for seed in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            splitting.thin(X, seed=seed)
    with pytest.raises(ValueError, match="channels"):
        splitting.split_deviance(X, np.ones((5, 2)), np.ones((2, 20)))
    with pytest.raises(ValueError, match="pixels"):
        splitting.split_deviance(X, np.ones((6, 2)), np.ones((2, 19)))
    with pytest.raises(ValueError, match="X has 20 channels"):   # (pixel-major: the 6 x 20 array is 6 pixels of 20 channels)
        splitting.split_deviance(X, np.ones((6, 2)), np.ones((2, 20)), layout="pm")
    with pytest.raises(NotImplementedError, match="33 components"):
        splitting.split_deviance(X, np.ones((6, 33)), np.ones((33, 20)))
    with pytest.raises(ValueError, match="log_shift"):
        splitting.split_deviance(X, np.ones((6, 2)), np.ones((2, 20)), log_shift=0)
    # what goes up: u8 and u16 as they are, other integers narrowed after the range check
    assert counts_image(X, "cm")[0] is X
    ok = X.astype(np.int64)
    ok[1, 1] = 255
    assert counts_image(ok, "cm")[0].dtype == np.uint8
    ok[1, 1] = 256
    got, n, p = counts_image(ok, "pm")
    assert got.dtype == np.uint16 and got[1, 1] == 256 and (n, p) == (20, 6)
    assert counts_image(torch.from_numpy(ok.astype(np.int32)), "cm")[0].dtype == torch.uint16


def test_no_cpu_fallback(lib, monkeypatch):
    import torch

    from espm_amd import splitting
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X = np.zeros((6, 20), np.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        splitting.thin(X)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        splitting.split_deviance(X, np.ones((6, 2)), np.ones((2, 20)))


def _est(**kw):
    from espm_amd.estimators import SmoothNMF
    args = dict(n_components=3, shape_2d=(4, 5), max_iter=5, verbose=0)
    args.update(kw)
    return SmoothNMF(**args)


def test_fit_split_refuses_before_any_upload(lib, monkeypatch):
    from espm_amd import splitting
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X = np.ones((6, 20), np.uint8)
    with pytest.raises(NotImplementedError, match="shard"):
        _est().shard(object()).fit_split(X)
    with pytest.raises(NotImplementedError, match="shard"):
        splitting.scan(X, [_est(), _est().shard(object())])
    with pytest.raises(TypeError, match="defined for counts"):
        _est().fit_split(X.astype(np.float32))
    with pytest.raises(ValueError, match="between 0 and 1"):
        _est().fit_split(X, q=1.0)
    with pytest.raises(ValueError, match="at least one"):
        splitting.scan(X, [])


def test_a_plain_fit_forgets_the_split(lib, monkeypatch):
    """fit_transform drops the split attributes first thing (the fit itself is cut short here: it needs the device)."""
    est = _est()
    for name in est._SPLIT_ATTRIBUTES:
        setattr(est, name, 1.0)
    assert set(est._SPLIT_ATTRIBUTES) == {"split_q_", "split_seed_", "heldout_deviance_", "train_deviance_", "heldout_deviance_map_",
                                          "train_deviance_map_", "heldout_counts_"}

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop

    monkeypatch.setattr(type(est), "_fit_validate", stop)
    with pytest.raises(Stop):
        est.fit_transform(np.ones((6, 20)))
    assert not any(hasattr(est, name) for name in est._SPLIT_ATTRIBUTES)


def test_adapter_routes_split_to_fit_split(lib):
    from espm_amd import hyperspy_adapter as ha

    class Est:
        hspy_comp, shape_2d = True, None

        def fit_split(self, X, q=0.8, seed=0):
            self.seen = (X.shape, q, seed)
            self.components_ = np.zeros((2, X.shape[1]))
            return np.zeros((X.shape[0], 2))

        def fit_transform(self, X):
            raise AssertionError("split was given")

        def fit_binned(self, X, bin):
            raise AssertionError("split was given")

    sig, est = ha.SpectrumImage(np.zeros((8, 12, 7), np.uint8)), Est()
    lr = ha.decompose(sig, est, split=(0.75, 9))
    assert est.seen == ((96, 7), 0.75, 9) and est.shape_2d == (8, 12)
    assert lr.loadings.shape == (96, 2) and lr.factors.shape == (7, 2) and lr.decomposition_algorithm is est
    with pytest.raises(ValueError, match="exclude each other"):
        ha.decompose(sig, Est(), split=(0.75, 9), bin=(2, 2))
    with pytest.raises(ValueError, match="exclude each other"):
        sig.decomposition(Est(), split=(0.75, 9), bin=(2, 2))
    with pytest.raises(ValueError, match=r"pair \(q, seed\)"):
        ha.decompose(sig, Est(), split=0.75)


def test_adapter_fills_the_results_of_a_foreign_signal(lib):
    import types

    from espm_amd import hyperspy_adapter as ha

    class Est:
        hspy_comp, shape_2d = True, None

        def fit_split(self, X, q=0.8, seed=0):
            self.seen = (X.shape, q, seed, X[13, 2])
            self.components_ = np.arange(2 * X.shape[1], dtype=np.float64).reshape(2, X.shape[1])
            return np.ones((X.shape[0], 2))

    cube = np.arange(8 * 12 * 7).reshape(8, 12, 7)
    sig = types.SimpleNamespace(data=cube, shape_2d=(8, 12), learning_results=ha.LearningResults(),
                                decomposition=lambda **k: pytest.fail("hyperspy's decomposition knows no split"))
    est = Est()
    lr = ha.decompose(sig, est, split=(0.5, 4))
    assert est.seen == ((96, 7), 0.5, 4, cube[1, 1, 2]) and est.shape_2d == (8, 12)
    assert lr is sig.learning_results and lr.output_dimension == 2 and np.array_equal(lr.factors, est.components_.T)
    with pytest.raises(TypeError, match="unsupported decomposition arguments with split"):
        ha.decompose(sig, Est(), split=(0.5, 4), output_dimension=2)
