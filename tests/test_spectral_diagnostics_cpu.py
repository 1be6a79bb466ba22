"""spectral_diagnostics without a device: the binding, the argument checks that come before any upload, the refusal to run without a
GPU, the host algebra from M to the error bars (measures.spectral_bounds) against the numpy reference, and the self-consistency of
that reference (tests/spectral_reference.py) and of its bounds."""
import ctypes as C

import numpy as np
import pytest

import diag_reference as dr
import spectral_reference as sr


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


def _call(f, x, layout, ld, n, p, k, ptr, scratch_bytes):
    return f(x, 0, layout, ld, n, p, ptr, ptr, k, 1e-14, ptr, ptr, ptr, ptr, ptr, scratch_bytes, None)


def test_entry_point_is_bound_and_the_wide_builds_refuse(lib):
    res, args = lib.SYMBOLS["espm_channel_diagnostics"]
    assert res is C.c_int and len(args) == 17
    res, args = lib.SYMBOLS["espm_channel_diagnostics_scratch"]
    assert res is C.c_size_t and len(args) == 3
    assert lib.CDIAG_PCHUNK >= 64 and lib.CDIAG_BLOCK == 256
    from espm_amd import _abi
    assert _abi.parse_defines(_abi.header_text())["ESPM_CDIAG_PCHUNK"] == lib.CDIAG_PCHUNK
    for k in (12, 20):   # the 9..16 and the 17..32 component builds export a stub
        v = lib.variant(k)
        rc = v.lib.espm_channel_diagnostics(None, 0, 0, 8, 8, 8, None, None, 3, 1e-14, None, None, None, None, None, 0, None)
        assert rc == lib.EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            v.check(rc)
        assert v.lib.espm_channel_diagnostics_scratch(8, 8, 3) == 0


def test_scratch_query(lib):
    q = lib.lib.espm_channel_diagnostics_scratch
    pc = lib.CDIAG_PCHUNK
    assert q(70, 64, 3) == 1 * (3 + 6) * 70 * 8
    assert q(70, pc, 8) == 1 * (3 + 36) * 70 * 8 and q(70, pc + 1, 8) == 2 * (3 + 36) * 70 * 8
    assert q(2048, 512 * 512, 5) == (512 * 512 // pc) * 18 * 2048 * 8
    assert q(0, 64, 3) == 0 and q(70, 64, 9) == 0


def test_host_side_argument_errors_need_no_device(lib):
    """Status codes of the narrow build's entry point for arguments it refuses before any launch."""
    f = lib.lib.espm_channel_diagnostics
    one = C.c_void_p(8)   # (never dereferenced: every call below is refused on the host)
    big = 1 << 30
    assert _call(f, one, 0, 8, 8, 8, 9, one, big) == lib.EUNSUPPORTED
    assert _call(f, one, 0, 8, 8, 8, 0, one, big) == lib.EUNSUPPORTED
    assert _call(f, None, 0, 8, 8, 8, 3, one, big) == lib.EINVAL
    assert _call(f, one, 0, 8, 8, 8, 3, None, big) == lib.EINVAL
    assert _call(f, one, 2, 8, 8, 8, 3, one, big) == lib.EINVAL          # layout
    assert _call(f, one, 0, 7, 8, 8, 3, one, big) == lib.EINVAL          # ld below the row length
    assert b"ld=7" in lib.lib.espm_mu_last_error()
    assert _call(f, one, 1, 7, 8, 16, 3, one, big) == lib.EINVAL         # pixel-major: rows of n
    assert _call(f, one, 0, 8, 0, 8, 3, one, big) == lib.EINVAL
    assert _call(f, one, 0, 8, 8, 0, 3, one, big) == lib.EINVAL
    need = lib.lib.espm_channel_diagnostics_scratch(8, 8, 3)
    assert _call(f, one, 0, 8, 8, 8, 3, one, need - 1) == lib.EINVAL     # a scratch that is too small
    msg = lib.lib.espm_mu_last_error()
    assert str(need).encode() in msg and str(need - 1).encode() in msg


def test_shape_checks_come_before_the_device(lib, monkeypatch):
    from espm_amd import measures
    from espm_amd import _image
    monkeypatch.setattr(_image, "on_device", lambda *a, **k: pytest.fail("the upload was reached"))
    X, D, H = np.zeros((6, 10), np.float32), np.ones((6, 2)), np.ones((2, 10))
    f = measures.spectral_diagnostics
    with pytest.raises(ValueError, match="layout"):
        f(X, D, H, layout="rows")
    with pytest.raises(ValueError, match="channels"):
        f(X, np.ones((5, 2)), H)
    with pytest.raises(ValueError, match="pixels"):
        f(X, D, np.ones((2, 9)))
    with pytest.raises(ValueError, match="channels"):
        f(X, D, H, layout="pm")
    with pytest.raises(ValueError, match="2-D"):
        f(np.zeros(6), D, H)
    with pytest.raises(ValueError, match="log_shift"):
        f(X, D, H, log_shift=0.0)
    with pytest.raises(NotImplementedError, match="9 components"):
        f(X, np.ones((6, 9)), np.ones((9, 10)))
    with pytest.raises(ValueError, match="G must be"):
        f(X, np.ones((4, 2)), H, G=np.ones((6, 3)))
    with pytest.raises(ValueError, match="channels"):
        f(X, np.ones((3, 2)), H, G=np.ones((5, 3)))
    with pytest.raises(ValueError, match="simplex_rows"):
        f(X, D, H, simplex_rows=[0, 6])
    with pytest.raises(ValueError, match="simplex_rows"):
        f(X, np.ones((3, 2)), H, G=np.ones((6, 3)), simplex_rows=[3])
    with pytest.raises(NotImplementedError, match="information matrix"):
        f(np.zeros((6, 10), np.float32), np.ones((300, 7)), np.ones((7, 10)), G=np.ones((6, 300)))


def test_no_cpu_fallback(lib, monkeypatch):
    import torch

    from espm_amd import measures
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    X, D, H, _ = dr.image(70, 64, 2, "float64", False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        measures.spectral_diagnostics(X, D, H)


def test_estimator_method_refuses_an_unfitted_estimator(lib):
    from sklearn.exceptions import NotFittedError

    from espm_amd.estimators import SmoothNMF
    with pytest.raises(NotFittedError):
        SmoothNMF(n_components=3).spectral_diagnostics(np.zeros((6, 10)))


def test_signal_axis_helper(lib):
    import types

    from espm_amd import hyperspy_adapter as ha
    est = types.SimpleNamespace(shape_2d=(4, 5))
    with pytest.raises(AttributeError, match="spectral_diagnostics"):
        ha.diagnostic_spectra(est)
    est.channel_deviance_, est.sum_spectrum_, est.model_spectrum_ = np.arange(7.0), np.arange(7.0) + 1, np.arange(7.0) + 2
    est.D_std_ = np.arange(21.0).reshape(7, 3)
    dev, xs, ys, band = ha.diagnostic_spectra(est)
    assert dev.shape == xs.shape == ys.shape == (7,) and band.shape == (3, 7) and band[1, 4] == est.D_std_[4, 1]
    sig = ha.SpectrumImage(np.zeros((4, 5, 7)))
    sig.learning_results.decomposition_algorithm = est
    assert sig.get_decomposition_diagnostic_spectra()[3].shape == (3, 7)


# ---- the reference itself -------------------------------------------------------------------------------------------------------
def _pchunk():
    from espm_amd import _abi
    return _abi.parse_defines(_abi.header_text())["ESPM_CDIAG_PCHUNK"]


# (n, p or None for "two chunks + 155", k, dtype): the GPU parity shapes
CASES = [(70, None, 3, "float32"), (70, None, 8, "uint8"), (308, 300, 5, "uint16"), (70, 64, 1, "float64"), (308, 667, 5, "uint8")]


def _p(p):
    return 2 * _pchunk() + 155 if p is None else p


@pytest.mark.parametrize("n,p,k,dtype", CASES)
def test_reference_images_meet_their_conditions(n, p, k, dtype):
    p = _p(p)
    X, D, H, facts = dr.image(n, p, k, dtype, False)
    assert not X[:, facts["empty_pixel"]].any() and not X[facts["zero_channel"]].any() and not D[facts["floor_channel"]].any()
    ref = sr.reference(X, D, H)
    assert ref["cond_max"] < 1e8, "the parity images must stay away from the NaN rule"
    assert np.isfinite(ref["W_std"]).all() and (ref["W_std"] > 0).all() and (ref["channel_deviance"] >= 0).all()
    fc = facts["floor_channel"]   # y is the floor there: M_c = H H^T / log_shift, and the one count gives x ln(x / log_shift)
    np.testing.assert_allclose(ref["M"][fc], (H @ H.T) / sr.LOG_SHIFT, rtol=1e-12)
    assert ref["channel_deviance"][fc] > 2 * (3 * np.log(3 / sr.LOG_SHIFT) - 3) - 1e-6
    if k > 1:
        Xg, G, W, Hg, _ = sr.dict_image(n, p, k, dtype)
        refg = sr.reference(Xg, W, Hg, G=G)
        assert refg["cond_max"] < 1e8 and np.isfinite(refg["W_std"]).all() and not refg["D_std"][facts["floor_channel"]].any()


def test_channel_and_pixel_deviance_sum_to_the_same():
    n, p, k = 70, 667, 3
    X, D, H, _ = dr.image(n, p, k, "float32", False)
    by_channel, by_pixel = sr.reference(X, D, H), dr.reference(X, D, H)
    total = by_pixel["deviance"].sum()
    assert abs(by_channel["channel_deviance"].sum() - total) <= 8 * n * p * dr.EPS * total


def test_constraint_removes_its_direction_and_never_widens_a_bar():
    n, p, k = 70, 300, 3
    X, D, H, _ = dr.image(n, p, k, "float32", False)
    free = sr.reference(X, D, H)
    for rows in (True, np.array([3, 10, 11, 40, 69])):
        con = sr.reference(X, D, H, simplex_rows=rows)
        idx = np.arange(n) if rows is True else rows
        S = free["C"]
        T = S[idx].sum(axis=0)
        Tinv = np.linalg.inv(T)
        # A^T C A = T - T T^-1 T in blocks: sum over the set of (S_c - S_c T^-1 S_c') summed over c, c'
        AtCA = T - T @ Tinv @ T
        assert np.abs(AtCA).max() <= 64 * k * k * dr.EPS * np.linalg.cond(T) * np.abs(T).max()
        assert (con["W_std"] <= free["W_std"] * (1 + 1e-12)).all(), "a constraint cannot widen an error bar"
        others = np.setdiff1d(np.arange(n), idx)
        assert np.array_equal(con["W_std"][others], free["W_std"][others])
        assert (con["W_std"][idx] < free["W_std"][idx]).mean() > 0.9   # (all but the floor channel, whose S_c is 1e-14 of the others')
    Xg, G, W, Hg, _ = sr.dict_image(n, p, k, "float32")
    freeg = sr.reference(Xg, W, Hg, G=G)
    for rows in (True, np.array([0, 2, 5])):
        con = sr.reference(Xg, W, Hg, G=G, simplex_rows=rows)
        A = np.zeros((sr.M_DICT, k, k))
        A[np.arange(sr.M_DICT) if rows is True else rows] = np.eye(k)
        A = A.reshape(-1, k)
        scale = np.abs(A.T @ freeg["C"] @ A).max()
        assert np.abs(A.T @ con["C"] @ A).max() <= 64 * (sr.M_DICT * k) ** 2 * dr.EPS * freeg["cond_max"] * scale
        assert (con["W_std"] <= freeg["W_std"] * (1 + 1e-12)).all() and (con["D_std"] <= freeg["D_std"] * (1 + 1e-12)).all()


def test_dictionary_path_with_identity_equals_the_identity_path():
    n, p, k = 70, 300, 3
    X, D, H, _ = dr.image(n, p, k, "float32", False)
    for rows in (None, True, np.array([3, 10, 11, 40, 69])):
        a = sr.reference(X, D, H, simplex_rows=rows)
        b = sr.reference(X, D, H, G=np.eye(n), simplex_rows=rows)
        np.testing.assert_allclose(b["W_std"], a["W_std"], rtol=1e-9)
        np.testing.assert_allclose(b["D_std"], a["D_std"], rtol=1e-9)


# ---- the bounds have room for the kernel's order of evaluation -------------------------------------------------------------------
def _kernel_order(X, D, H, log_shift=sr.LOG_SHIFT, dtype=np.float64):
    """The sums as the kernel forms them: t = y - x + x ln(x (1 / y)) and h_i (1 / y) h_j, added pixel by pixel inside a chunk of
    ESPM_CDIAG_PCHUNK pixels, the chunks added afterwards in ascending order."""
    x, D, H = (np.asarray(a).astype(dtype) for a in (X, D, H))
    k = H.shape[0]
    Y = np.maximum(D @ H, dtype(log_shift))
    w = 1 / Y
    t = Y - x
    pos = x > 0
    t[pos] += x[pos] * np.log(x[pos] * w[pos])
    il, jl = np.tril_indices(k)
    terms = dict(dev=t, xs=x, ys=Y)
    for a, (i, j) in enumerate(zip(il, jl)):
        terms[a] = (H[i][None, :] * w) * H[j][None, :]
    out = {}
    pc = _pchunk()
    for name, v in terms.items():
        parts = [np.cumsum(v[:, a:a + pc], axis=1)[:, -1] for a in range(0, v.shape[1], pc)]   # (cumsum adds in order)
        out[name] = np.cumsum(np.stack(parts, axis=1), axis=1)[:, -1]
    M = np.empty((x.shape[0], k, k), dtype=dtype)
    for a, (i, j) in enumerate(zip(il, jl)):
        M[:, i, j] = M[:, j, i] = out[a]
    return dict(channel_deviance=2 * out["dev"], sum_spectrum=out["xs"], model_spectrum=out["ys"], M=M)


@pytest.mark.parametrize("n,p,k,dtype", CASES)
def test_bounds_hold_for_the_kernels_order_of_evaluation(lib, n, p, k, dtype):
    from espm_amd import measures
    p = _p(p)
    X, D, H, _ = dr.image(n, p, k, dtype, False)
    integer = dtype != "float64"
    for rows in (None, True):
        ref = sr.reference(X, D, H, simplex_rows=rows)
        emu = _kernel_order(X, D, H)
        emu.update(measures.spectral_bounds(emu["M"], simplex_rows=rows))
        assert emu["n_singular"] == 0
        sr.check(emu, ref, p, k, f"n={n} p={p} k={k} {dtype} rows={rows}: kernel order", integer=integer)
        if np.finfo(np.longdouble).eps < 2.0 ** -60:
            wide = {a: np.asarray(v, dtype=np.float64) for a, v in _kernel_order(X, D, H, dtype=np.longdouble).items()}
            for name, got in (("reference", dict(ref)), ("kernel order", emu)):
                sr.check(dict(got, W_std=ref["W_std"], D_std=ref["D_std"]), dict(ref, **wide), p, k,
                         f"    {name} vs extended precision", integer=integer)
    if k > 1:
        Xg, G, W, Hg, _ = sr.dict_image(n, p, k, dtype)
        for rows in (None, True, np.array([0, 2, 5])):
            ref = sr.reference(Xg, W, Hg, G=G, simplex_rows=rows)
            emu = _kernel_order(Xg, G @ W, Hg)
            emu.update(measures.spectral_bounds(emu["M"], G=G, simplex_rows=rows))
            sr.check(emu, ref, p, k, f"n={n} p={p} k={k} {dtype} dictionary rows={rows}: kernel order", integer=integer)


# ---- the host algebra of measures on seeded M ------------------------------------------------------------------------------------
def _seeded_M(n, k, seed):
    rng = np.random.default_rng(seed)
    B = rng.random((n, k, 3 * k)) + 0.1
    return np.einsum("cik,cjk->cij", B, B)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_spectral_bounds_against_the_reference(lib, k):
    from espm_amd import measures
    n, m = 40, sr.M_DICT
    M = _seeded_M(n, k, 5 + k)
    rng = np.random.default_rng(17)
    G = rng.random((n, m)) + 0.05
    for G_, rows_list in ((None, (None, True, np.array([1, 4, 5, 30]), [4, 1, 1])), (G, (None, True, np.array([0, 3]), [3, 0]))):
        for rows in rows_list:
            ref = sr.bounds_from_M(M, G=G_, simplex_rows=None if rows is None else True if rows is True else np.unique(rows))
            got = measures.spectral_bounds(M, G=G_, simplex_rows=rows)
            assert got["n_singular"] == 0 and got["W_std"].shape == ((n, k) if G_ is None else (m, k)) and got["D_std"].shape == (n, k)
            for name, cond in (("W_std", "cond"), ("D_std", "cond_D")):   # (the entry's own cond(M_c), or cond(F))
                r = np.max(np.abs(got[name] - ref[name]) / (64 * k * dr.EPS * ref[cond] * ref[name]))
                print(f"k={k} G={'yes' if G_ is not None else 'no'} rows={rows}: {name} {r:.3g} of 64 k eps cond")
                assert r <= 1


def test_spectral_bounds_singular_cases(lib):
    from espm_amd import measures
    n, k = 40, 3
    M = _seeded_M(n, k, 3)
    v = np.array([1.0, 2.0, 3.0])
    M[7] = np.outer(v, v)   # rank one: a pivot at rounding level
    free = measures.spectral_bounds(M)
    assert free["n_singular"] == 1 and np.isnan(free["W_std"][7]).all() and np.isfinite(np.delete(free["W_std"], 7, axis=0)).all()
    clean = sr.bounds_from_M(np.delete(M, 7, axis=0))
    np.testing.assert_allclose(np.delete(free["W_std"], 7, axis=0), clean["W_std"], rtol=1e-10)
    # under the simplex the singular row is left out of the sum: the others are bounded as if it were held
    con = measures.spectral_bounds(M, simplex_rows=True)
    clean = sr.bounds_from_M(np.delete(M, 7, axis=0), simplex_rows=True)
    assert con["n_singular"] == 1 and np.isnan(con["W_std"][7]).all()
    np.testing.assert_allclose(np.delete(con["W_std"], 7, axis=0), clean["W_std"], rtol=1e-9)
    # a singular F: two identical columns of G
    G = np.random.default_rng(1).random((n, 4)) + 0.05
    G[:, 3] = G[:, 1]
    for rows in (None, True):
        out = measures.spectral_bounds(_seeded_M(n, k, 4), G=G, simplex_rows=rows)
        assert out["n_singular"] == 4 and np.isnan(out["W_std"]).all() and np.isnan(out["D_std"]).all()
    # k = 1 on the simplex over one row: that entry has no freedom
    one = measures.spectral_bounds(_seeded_M(5, 1, 9), simplex_rows=[2])
    assert one["W_std"][2, 0] == 0 and (np.delete(one["W_std"], 2, axis=0) > 0).all()
