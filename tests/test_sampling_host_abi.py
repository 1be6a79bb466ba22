"""The host half of the two sampling entry points (include/espm_mu.h, "Poisson sampling") refuses what it must BEFORE anything reaches a
device (no GPU needed), with the offending values in espm_mu_last_error(); the wide builds export them as stubs.  The pointers handed
over are never dereferenced: every call below is refused on the host."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


U8, U16, CM, PM = 0, 1, 0, 1
TOP = 2 ** 32 - 2


def _vp(v):
    return None if v is None else C.c_void_p(v)


def _sample(f, d=8, h=8, k=3, n=8, p=80, p_total=80, j0=0, seed=0, replicate=0, x=8, dtype=U16, layout=CM, ld=80, counts=8):
    return f(_vp(d), _vp(h), k, n, p, p_total, j0, seed, replicate, _vp(x), dtype, layout, ld, _vp(counts), None)


def _dev(f, d=8, h=8, k=3, n=8, p=80, p_total=80, j0=0, seed=0, replicate0=0, n_rep=4, log_shift=1e-14, dev=8):
    return f(_vp(d), _vp(h), k, n, p, p_total, j0, seed, replicate0, n_rep, log_shift, _vp(dev), None)


def test_poisson_sample_argument_errors_need_no_device(lib):
    f, err = lib.lib.espm_poisson_sample, lib.lib.espm_mu_last_error
    assert _sample(f, d=None, h=None, x=None, counts=None) == lib.EINVAL      # the null call
    for name in ("d", "h", "x", "counts"):
        assert _sample(f, **{name: None}) == lib.EINVAL, name
    assert _sample(f, k=0) == lib.EINVAL and b"k=0" in err()
    assert _sample(f, k=33) == lib.EINVAL and b"k=33" in err()
    assert _sample(f, n=0) == lib.EINVAL and b"n=0" in err()
    assert _sample(f, p=0, p_total=0) == lib.EINVAL and b"p=0" in err()
    assert _sample(f, p_total=79) == lib.EINVAL and b"p_total=79" in err()                # the image is smaller than its slab
    assert _sample(f, p_total=100, j0=21) == lib.EINVAL and b"j0=21" in err()             # the slab ends behind the image
    assert _sample(f, p_total=100, j0=-1) == lib.EINVAL and b"j0=-1" in err()
    assert _sample(f, p_total=1 << 62) == lib.EINVAL and b"64-bit" in err()               # n x p_total overflows the index
    assert _sample(f, ld=79) == lib.EINVAL and b"ld=79" in err()
    assert _sample(f, layout=PM, ld=7) == lib.EINVAL and b"ld=7" in err()                 # pixel-major: rows of n
    assert _sample(f, dtype=2) == lib.EINVAL and b"x_dtype 2" in err()                    # counts only
    assert _sample(f, dtype=3) == lib.EINVAL and _sample(f, dtype=-1) == lib.EINVAL
    assert _sample(f, layout=2) == lib.EINVAL and b"x_layout 2" in err()
    assert _sample(f, replicate=TOP + 1) == lib.EINVAL and b"replicate=4294967295" in err()
    assert _sample(f, replicate=-1) == lib.EINVAL and b"replicate=-1" in err()
    with pytest.raises(ValueError):
        lib.check(lib.EINVAL)


def test_sample_deviance_argument_errors_need_no_device(lib):
    f, err = lib.lib.espm_sample_deviance, lib.lib.espm_mu_last_error
    assert _dev(f, d=None, h=None, dev=None) == lib.EINVAL                                # the null call
    for name in ("d", "h", "dev"):
        assert _dev(f, **{name: None}) == lib.EINVAL, name
    assert _dev(f, k=0) == lib.EINVAL and b"k=0" in err()
    assert _dev(f, k=33) == lib.EINVAL and b"k=33" in err()
    assert _dev(f, n=0) == lib.EINVAL and _dev(f, p=0) == lib.EINVAL
    assert _dev(f, p_total=100, j0=21) == lib.EINVAL and b"j0=21" in err()
    assert _dev(f, p_total=1 << 62) == lib.EINVAL and b"64-bit" in err()
    assert _dev(f, n_rep=0) == lib.EINVAL and b"n_rep=0" in err()
    assert _dev(f, n_rep=-3) == lib.EINVAL and b"n_rep=-3" in err()
    assert _dev(f, replicate0=TOP - 2, n_rep=4) == lib.EINVAL and b"4294967295" in err()  # the last replicate is past 2^32 - 2
    assert _dev(f, replicate0=-1) == lib.EINVAL and b"replicate=-1" in err()
    assert _dev(f, replicate0=2 ** 63 - 1) == lib.EINVAL
    assert _dev(f, log_shift=0.0) == lib.EINVAL and b"log_shift=0" in err()
    assert _dev(f, log_shift=-1.0) == lib.EINVAL and _dev(f, log_shift=float("nan")) == lib.EINVAL


def test_the_wide_builds_export_stubs(lib):
    for k in (12, 20):
        v = lib.variant(k)
        rc = v.lib.espm_poisson_sample(None, None, k, 8, 8, 8, 0, 0, 0, None, U16, CM, 8, None, None)
        assert rc == lib.EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            v.check(rc)
        assert v.lib.espm_sample_deviance(None, None, k, 8, 8, 8, 0, 0, 0, 4, 1e-14, None, None) == lib.EUNSUPPORTED
