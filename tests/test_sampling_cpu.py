"""Poisson sampling without a device: the table of the unit draw re-derived, the rule in numpy (tests/sampling_reference.py) as a
Poisson sampler, ``calibrate`` against hand-computed values, the binding, and what ``sample``, ``null_deviance`` and the estimator's
``simulate`` / ``calibrate_deviance`` / ``bootstrap`` refuse before anything is uploaded."""

import numpy as np
import pytest

from abi_header import CTYPE, _declared
import sampling_reference as sref
import splitting_reference as sr


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


# ---- the table -----------------------------------------------------------------------------------------------------------------------
def test_unit_cdf_is_the_exact_table(lib):
    """T_i = floor(2^32 sum_{j <= i} e^-1 / j!) with 60-digit decimals: e^-1 from its alternating series (term 60 is below 1e-81)."""
    import decimal

    from espm_amd import sampling
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        one = decimal.Decimal(1)
        term, einv = one, decimal.Decimal(0)
        for j in range(60):
            einv += term if j % 2 == 0 else -term
            term = term / (j + 1)
        table, cdf, fact = [], decimal.Decimal(0), one
        for i in range(12):
            if i:
                fact *= i
            cdf += einv / fact
            table.append(int((cdf * (1 << 32)).to_integral_value(rounding=decimal.ROUND_FLOOR)))
    assert tuple(table) == tuple(sampling.UNIT_CDF) == tuple(int(v) for v in sref.UNIT_CDF)
    assert " ".join(f"{v:08x}" for v in table) == ("5e2d58d8 bc5ab1b1 eb715e1d fb239797 ff1025f5 ffd90f3b fffa8b71 ffff540c ffffed1f fffffe21 "
                                                   "ffffffd4 fffffffc")
    # the unit draw's moments, from the table itself: mean 1 + 1.4e-9, variance 1 + 1.3e-8
    pmf = np.diff(np.array([0] + table + [1 << 32], dtype=np.float64)) / 2.0 ** 32
    mean = float((pmf * np.arange(13)).sum())
    var = float((pmf * np.arange(13) ** 2).sum()) - mean ** 2
    assert abs(mean - 1) < 3e-9 and abs(var - 1) < 3e-8
    # the header writes the table out too
    from espm_amd import _abi
    assert "5e2d58d8 bc5ab1b1 eb715e1d fb239797 ff1025f5 ffd90f3b fffa8b71 ffff540c ffffed1f fffffe21 ffffffd4 fffffffc" in _abi.header_text()


def test_unit_draw_of_the_reference():
    w = np.array([0, 0x5e2d58d7, 0x5e2d58d8, 0xbc5ab1b1, 0xfffffffb, 0xfffffffc, 0xffffffff], dtype=np.uint32)
    assert sref.unit(w).tolist() == [0, 0, 1, 2, 11, 12, 12]


# ---- the rule as a sampler --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.6, 17.25])
def test_reference_rule_is_poisson(rate):
    """10^5 entries at one rate: the sample mean within 5 sigma of the rate (sigma^2 = rate / N), the sample variance within 5 sigma
    of it (for a Poisson variable var(s^2) = (rate + 2 rate^2) / N up to 1 / N^2)."""
    N = 100000
    X, info = sref.sample_rates(np.full((100, 1000), rate), seed=2024, replicate=1)
    assert info == dict(saturated=0, invalid=0) and X.dtype == np.uint16
    x = X.astype(np.float64)
    z_mean = (x.mean() - rate) / np.sqrt(rate / N)
    z_var = (x.var(ddof=1) - rate) / np.sqrt((rate + 2 * rate ** 2) / N)
    print(f"rate {rate}: mean at {z_mean:+.2f} sigma, variance at {z_var:+.2f} sigma")
    assert abs(z_mean) < 5 and abs(z_var) < 5


def _small(k=3):
    D, H = sr.model(24, 200, k)
    return D, H


def test_reference_rates_are_the_plain_loop():
    D, H = _small()
    y = sref.rates(D, H)
    c, j = 5, 17
    acc = 0.0
    for i in range(3):
        acc = acc + float(D[c, i]) * float(H[i, j])
    assert y[c, j] == acc and np.allclose(y, D @ H, rtol=1e-15, atol=0)
    assert (y[:, 11] == 0).all()


def test_a_slab_is_its_slice_and_the_geometry_matters():
    D, H = _small()
    X, _ = sref.sample(D, H, 7, 3)
    S, _ = sref.sample(D, np.ascontiguousarray(H[:, 50:120]), 7, 3, p_total=200, j0=50)
    assert np.array_equal(S, X[:, 50:120])
    assert not np.array_equal(sref.sample(D, np.ascontiguousarray(H[:, 50:120]), 7, 3)[0], S)


def test_replicates_and_seeds_differ():
    D, H = _small()
    A = sref.sample(D, H, 0, 0)[0]
    assert np.array_equal(A, sref.sample(D, H, 0, 0)[0])
    for seed, rep in ((0, 1), (1, 0), (1 << 32, 0), (0, 2 ** 32 - 2)):
        assert not np.array_equal(A, sref.sample(D, H, seed, rep)[0]), (seed, rep)


def test_reference_extremes():
    """0 and 1e-14 draw (almost surely) nothing; an exact integer has thr = 0; above 65535 saturates without a draw; a negative or NaN
    rate is invalid; 8 bits saturate at 255."""
    y = np.array([[0.0, 1e-14, 7.0, 255.5, 300.25, 65535.0, 65536.5, -1.0, np.nan, np.inf]])
    X, info = sref.sample_rates(y, 5, 0)
    assert X[0, 0] == 0 and X[0, 1] == 0 and X[0, 6] == 65535 and X[0, 7] == X[0, 8] == X[0, 9] == 0
    assert info["invalid"] == 3 and info["saturated"] == 1 + int(X[0, 5] == 65535)
    assert abs(int(X[0, 3]) - 255.5) < 5 * 16 and abs(int(X[0, 4]) - 300.25) < 5 * 17.4
    X8, info8 = sref.sample_rates(y, 5, 0, dtype=np.uint8)
    assert X8[0, 4] == 255 and X8[0, 5] == 255 and X8[0, 6] == 255 and np.array_equal(np.minimum(X, 255)[0, :3], X8[0, :3])
    assert info8["saturated"] == int((np.minimum(X.astype(np.int64), 256)[0] > 255).sum())
    # the pieces are words of their own: 7.0 is seven unit draws of blocks 4 and 5, no word of block 0
    w4 = sr.philox4x32((2, 0, 4, 1), (5, 0))
    w5 = sr.philox4x32((2, 0, 5, 1), (5, 0))
    assert int(X[0, 2]) == int(sum(sref.unit(w4[t]) for t in range(4)) + sum(sref.unit(w5[t]) for t in range(3)))


def test_reference_deviance_and_its_bound():
    D, H = _small()
    X, _ = sref.sample(D, H, 1, 0)
    ref = sref.deviance(X, D, H)
    Y = np.maximum(D @ H, sref.LOG_SHIFT)
    x = X.astype(np.float64)
    t = np.where(x > 0, x * np.log(np.where(x > 0, x, 1) / Y), 0.0) - x + Y
    assert np.allclose(ref["map"], 2 * t.sum(axis=0), rtol=1e-12)
    assert np.isfinite(ref["map"]).all() and abs(ref["map"][11] - 48 * sref.LOG_SHIFT) < 1e-26   # (pixel 11: at the floor, no counts)
    assert (ref["bound"] > 0).all() and (ref["bound"] < 1e-9 * np.maximum(ref["map"], 1)).all()


# ---- calibrate -------------------------------------------------------------------------------------------------------------------------
def test_calibrate_against_hand_computed_values(lib):
    from espm_amd import sampling
    null = np.array([[1.0, 10.0], [2.0, 10.0], [3.0, 13.0], [6.0, 15.0]])
    dev = np.array([3.0, 20.0])
    out = sampling.calibrate(dev, null)
    assert np.array_equal(out["null_mean"], [3.0, 12.0])
    # ddof = 1: ((4 + 1 + 0 + 9) / 3, (4 + 4 + 1 + 9) / 3)
    assert np.allclose(out["null_std"], [np.sqrt(14.0 / 3.0), np.sqrt(6.0)], rtol=1e-15)
    assert np.allclose(out["z"], [0.0, 8.0 / np.sqrt(6.0)], rtol=1e-15, atol=0)
    assert np.array_equal(out["pvalue"], [(1 + 2) / 5, 1 / 5])   # (3.0 and 6.0 reach 3.0; nothing reaches 20)
    with pytest.raises(ValueError, match="replicates"):
        sampling.calibrate(dev, null[:1])
    with pytest.raises(ValueError, match="pixels"):
        sampling.calibrate(dev[:1], null)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["espm_poisson_sample", "espm_sample_deviance"])
def test_symbols_are_bound_with_the_headers_signatures(lib, name):
    res, args = lib.SYMBOLS[name]
    cres, cargs = _declared(name)
    assert res is CTYPE[cres]
    assert list(args) == [CTYPE[a] for a in cargs]
    for k in (3, 12, 20):
        assert hasattr(lib.variant(k).lib, name)


def test_header_and_packaged_copy_carry_the_sizes(lib):
    import os

    from espm_amd import _abi, sampling
    d = _abi.parse_defines(_abi.header_text())
    assert d["ESPM_SAMPLE_BLOCK"] == lib.SAMPLE_BLOCK == 256 and d["ESPM_SAMPLE_HEAVY"] == lib.SAMPLE_HEAVY == 256 == sref.HEAVY
    assert d["ESPM_SAMPLE_MAX_RATE"] == lib.SAMPLE_MAX_RATE == sampling.MAX_RATE == 65535
    assert d["ESPM_SAMPLE_MAX_K"] == lib.SAMPLE_MAX_K == sampling.MAX_K == 32
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert open(os.path.join(root, "include", "espm_mu.h")).read() == open(os.path.join(root, "espm_amd", "include", "espm_mu.h")).read()


# ---- the Python module, before the device -------------------------------------------------------------------------------------------
def test_sample_raises_before_upload(lib, monkeypatch):
    from espm_amd import sampling
    monkeypatch.setattr(sampling, "_upload", lambda *a, **k: pytest.fail("the upload was reached"))
    D, H = np.ones((6, 2)), np.ones((2, 20))
    for f in (sampling.sample, sampling.null_deviance):
        with pytest.raises(ValueError, match="components"):
            f(np.ones((6, 3)), H)
        with pytest.raises(ValueError, match="components"):
            f(np.ones(6), H)
        with pytest.raises(ValueError, match="not finite"):
            f(np.where(np.arange(12).reshape(6, 2) == 3, np.nan, 1.0), H)
        with pytest.raises(ValueError, match="not finite"):
            f(D, np.where(np.arange(40).reshape(2, 20) == 7, np.inf, 1.0))
        with pytest.raises(ValueError, match="negative"):
            f(D, -H)
        with pytest.raises(NotImplementedError, match="33 components"):
            f(np.ones((6, 33)), np.ones((33, 20)))
        for seed in (-1, 1 << 64, 0.5, True):
            with pytest.raises(ValueError, match="seed"):
                f(D, H, seed=seed)
    for rep in (-1, 2 ** 32 - 1, 0.5, True):
        with pytest.raises(ValueError, match="replicate"):
            sampling.sample(D, H, replicate=rep)
    with pytest.raises(ValueError, match="replicate"):
        sampling.null_deviance(D, H, n_rep=3, replicate0=2 ** 32 - 3)   # (the last one would be 2^32 - 1)
    for n_rep in (0, -2, 1.5):
        with pytest.raises(ValueError, match="n_rep"):
            sampling.null_deviance(D, H, n_rep=n_rep)
    with pytest.raises(ValueError, match="log_shift"):
        sampling.null_deviance(D, H, log_shift=0.0)
    with pytest.raises(ValueError, match="dtype"):
        sampling.sample(D, H, dtype=np.float32)
    with pytest.raises(ValueError, match="dtype"):
        sampling.sample(D, H, dtype=np.int16)
    with pytest.raises(ValueError, match="layout"):
        sampling.sample(D, H, layout="rows")
    assert sampling._check_replicate(2 ** 32 - 2) == 2 ** 32 - 2 and sampling._check_replicate(2 ** 32 - 4, 3) == 2 ** 32 - 4


def test_no_cpu_fallback(lib, monkeypatch):
    import torch

    from espm_amd import sampling
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    D, H = np.ones((6, 2)), np.ones((2, 20))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sampling.sample(D, H)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sampling.null_deviance(D, H, n_rep=2)


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

    from espm_amd import measures, sampling
    monkeypatch.setattr(sampling, "_upload", lambda *a, **k: pytest.fail("the upload was reached"))
    monkeypatch.setattr(measures, "pixel_diagnostics", lambda *a, **k: pytest.fail("the diagnostics were reached"))
    calls = {"simulate": lambda e: e.simulate(), "calibrate_deviance": lambda e: e.calibrate_deviance(), "bootstrap": lambda e: e.bootstrap()}
    from espm_amd.estimators import SmoothNMF
    for name, call in calls.items():
        with pytest.raises(NotFittedError):
            call(SmoothNMF(n_components=3, verbose=0))
        with pytest.raises(NotImplementedError, match=name + " does not cover shard"):
            call(_fitted().shard(object()))
        binned = _fitted()
        binned.bin_ = (2, 2)
        with pytest.raises(ValueError, match="fit_binned"):
            call(binned)
        with pytest.raises(NotImplementedError, match="33 components"):
            call(_fitted(n_components=33))
    est = _fitted()
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            est.simulate(seed=seed)
        with pytest.raises(ValueError, match="seed"):
            est.calibrate_deviance(seed=seed)
        with pytest.raises(ValueError, match="seed"):
            est.bootstrap(seed=seed)
    with pytest.raises(ValueError, match="replicate"):
        est.simulate(replicate=2 ** 32 - 1)
    with pytest.raises(ValueError, match="at least two"):
        est.calibrate_deviance(n_rep=1)
    with pytest.raises(ValueError, match="at least two"):
        est.bootstrap(n_boot=1)
    with pytest.raises(ValueError, match="n_rep"):
        est.bootstrap(n_boot=0)
    with pytest.raises(NotImplementedError, match="12 components"):   # (the diagnostics' limit)
        _fitted(n_components=12).calibrate_deviance()


def test_bootstrap_copy_and_start(lib):
    est = _fitted(normalize=True, fixed_W=-np.ones((6, 3)), G=None, mu=0.3, lambda_L=2.0)
    est.norm_factor_ = 4.0
    est.set_precision("fp64")
    boot = est._bootstrap_copy(max_iter=7)
    assert type(boot) is type(est) and boot is not est and not hasattr(boot, "W_")
    assert boot.max_iter == 7 and est.max_iter == 5 and boot._fp64() and boot.fixed_W is est.fixed_W and boot.shape_2d == (4, 5)
    params, mine = boot.get_params(), est.get_params()
    assert set(params) == set(mine) and all(params[n] == mine[n] for n in ("mu", "lambda_L", "normalize", "n_components", "simplex_H"))
    W0, H0 = est._bootstrap_start()
    assert np.array_equal(W0, 4.0 * est.W_) and np.array_equal(H0, est.H_)
    assert not _fitted()._bootstrap_copy()._fp64() and _fitted()._bootstrap_copy().max_iter == 5


def test_adapter_maps(lib):
    import types

    from espm_amd import hyperspy_adapter as ha
    est = types.SimpleNamespace(shape_2d=(4, 5))
    with pytest.raises(AttributeError, match="calibrate_deviance"):
        ha.calibrated_deviance_maps(est)
    with pytest.raises(AttributeError, match="bootstrap"):
        ha.bootstrap_maps(est)
    est.deviance_z_, est.deviance_pvalue_, est.H_boot_std_ = np.arange(20.0), np.arange(20.0) / 20, np.arange(60.0).reshape(3, 20)
    z, pv = ha.calibrated_deviance_maps(est)
    assert z.shape == pv.shape == (4, 5) and z[1, 2] == 7.0 and pv[3, 4] == 19 / 20
    assert ha.bootstrap_maps(est).shape == (3, 4, 5) and ha.bootstrap_maps(est)[2, 1, 0] == 45.0

    class Est:
        hspy_comp, shape_2d = False, (4, 5)

        def simulate(self, seed=0, replicate=0):
            self.seen = (seed, replicate)
            return np.arange(6 * 20, dtype=np.uint16).reshape(6, 20)

    e = Est()
    sig = ha.SpectrumImage.simulate(e, seed=3, replicate=2)
    assert isinstance(sig, ha.SpectrumImage) and sig.data.shape == (4, 5, 6) and e.seen == (3, 2)
    assert np.array_equal(sig.X, np.arange(6 * 20).reshape(6, 20)) and sig.data.dtype == np.uint16
