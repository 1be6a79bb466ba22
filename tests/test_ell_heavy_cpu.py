"""Heavy elements of the sparse count store (include/espm_mu.h, ell_hv_*): integer counts from 256 to 2^24 stay out of the 16-bit lists
and are kept with their exact values in two orders.  The tensor-op builder on host tensors, and the C ABI's refusal of a heavy set it
cannot use (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import _lib
    return _lib


def _image(p, n, seed, heavy=0.005):
    rng = np.random.default_rng(seed)
    X = rng.poisson(0.3, size=(p, n)).astype(np.float64)
    nz = np.flatnonzero(X)
    pick = rng.choice(nz, size=max(1, int(heavy * nz.size)), replace=False)
    X.flat[pick] = rng.integers(256, 60001, size=pick.size)
    X[3, :] = 0
    X[3, [5, 9]] = [256, 1 << 24]             # a pixel whose only counts are heavy (the smallest and the largest)
    X[:, 7] = 0
    X[[0, p - 1], 7] = [300, 4000]            # a channel whose only counts are heavy
    return torch.from_numpy(X)


@pytest.mark.parametrize("p,n,tile", [(700, 90, 128), (1500, 300, 512), (256, 4100, 64)])
def test_heavy_set_holds_exactly_the_large_counts(lib, p, n, tile):
    from espm_amd import ell
    X = _image(p, n, seed=p + n)
    p_pad = (p + 511) // 512 * 512
    out = ell.build(X, p_pad, max(1, (n - 1).bit_length()), tile)
    hv = out["hv"]
    heavy = (X >= 256).nonzero()
    assert hv["n"] == heavy.shape[0] and hv["npx"] == int(torch.unique(heavy[:, 0]).numel())
    # pixel-major order decodes back to the heavy elements, with their values
    px, off, pm = hv["px"].long(), hv["px_off"].long(), hv["pm"].long()
    assert torch.equal(px, torch.unique(heavy[:, 0]))
    q = torch.repeat_interleave(px, off[1:] - off[:-1])
    D = torch.zeros_like(X)
    D[q, pm[:, 0]] = pm[:, 1].double()
    assert torch.equal(D, torch.where(X >= 256, X, torch.zeros_like(X)))
    assert torch.equal(torch.stack((q, pm[:, 0]), 1), heavy)          # by pixel, then channel
    # (W block, channel) order: the same elements, groups by block then channel, pixels ascending inside a group
    pb = 2 * tile
    grp, goff, wm = hv["grp"].long(), hv["grp_off"].long(), hv["wm"].long()
    assert hv["ngrp"] == grp.numel() == goff.numel() - 1 and int(goff[-1]) == hv["n"]
    c = torch.repeat_interleave(grp, goff[1:] - goff[:-1])
    Dw = torch.zeros_like(X)
    Dw[wm[:, 0], c] = wm[:, 1].double()
    assert torch.equal(Dw, D)
    key = (wm[:, 0] // pb) * n + c
    assert bool((key[1:] >= key[:-1]).all())
    same = key[1:] == key[:-1]
    assert bool((wm[1:, 0][same] > wm[:-1, 0][same]).all())
    gfirst = wm[goff[:-1], 0] // pb
    assert bool(((wm[goff[1:] - 1, 0] // pb) == gfirst).all())     # a group stays inside its W block
    assert int(X[3].count_nonzero()) == 2 and X[3, 9] == 1 << 24 and D[3, 9] == 1 << 24


@pytest.mark.parametrize("tile", [64, 512])
def test_lists_are_those_of_the_image_without_its_heavy_elements(lib, tile):
    from espm_amd import ell
    p, n = 1200, 150
    X = _image(p, n, seed=11)
    light = torch.where(X >= 256, torch.zeros_like(X), X)
    a = ell.build(X, 1536, 8, tile)
    b = ell.build(light, 1536, 8, tile)
    assert "hv" in a and "hv" not in b
    for key in ("ell_h", "ell_h_off", "klc", "pix_perm", "ell_w", "ell_w_off", "chan_perm"):
        assert torch.equal(a[key], b[key]), key
    for key in ("n_cg", "nblk_w", "entries_h", "entries_w", "rows_h", "rows_w", "unit_rows_h", "unit_rows_w"):
        assert a[key] == b[key], key
    assert a["nnz"] == b["nnz"] + a["hv"]["n"] == int(X.count_nonzero())


def test_an_image_of_small_counts_has_no_heavy_set(lib):
    from espm_amd import ell
    X = torch.from_numpy(np.minimum(np.random.default_rng(5).poisson(2.0, size=(600, 80)), 255).astype(np.float32))
    X[0, 0] = 255
    out = ell.build(X, 1024, 7, 128)
    assert set(out) == {"ell_h", "ell_h_off", "klc", "pix_perm", "ell_w", "ell_w_off", "chan_perm", "n_cg", "nblk_w", "nnz", "entries_h",
                        "entries_w", "rows_h", "rows_w", "unit_rows_h", "unit_rows_w"}
    assert ell.split_heavy(X, 256)[1] is None


def _queried(lib, x_dtype):
    st = lib.MUState()
    st.n, st.p, st.k, st.x_dtype = 64, 1000, 3, x_dtype
    assert lib.lib.espm_mu_query(C.byref(st)) == 0
    st.xscale = 1.0
    return st


def _fake_ptrs(st, names):
    keep = []
    for name in names:
        buf = C.create_string_buffer(64)
        keep.append(buf)
        setattr(st, name, C.addressof(buf))
    return keep


def test_abi_refuses_a_heavy_set_it_cannot_use(lib):
    hv_ptrs = ("ell_hv_px", "ell_hv_px_off", "ell_hv_pm", "ell_hv_klc", "ell_hv_kl", "ell_hv_grp", "ell_hv_grp_off", "ell_hv_wm", "ell_fill_num")
    # a dense store with a heavy set
    st = _queried(lib, lib.X_F32)
    keep = _fake_ptrs(st, hv_ptrs)
    st.ell_hv_n, st.ell_hv_npx, st.ell_hv_ngrp = 4, 2, 3
    for name in ("espm_mu_step_h", "espm_mu_step_hw", "espm_mu_w_accum", "espm_mu_iterate", "espm_mu_loss_only"):
        res, argtypes = lib.SYMBOLS[name]
        args = [C.c_int(0)] * (len(argtypes) - 2) + [None]
        assert getattr(lib.lib, name)(C.byref(st), *args) == lib.EINVAL, name
        assert b"ell_hv_n" in lib.lib.espm_mu_last_error(), name
    # the sparse store with NULL heavy arrays
    st = _queried(lib, lib.X_ELL)
    keep += _fake_ptrs(st, ("ell_h", "ell_h_off", "ell_klc", "ell_w", "ell_w_off", "chan_perm", "pix_perm"))
    st.ell_hv_n, st.ell_hv_npx, st.ell_hv_ngrp = 4, 2, 3
    for missing in hv_ptrs:
        keep += _fake_ptrs(st, [n for n in hv_ptrs if n != missing])
        setattr(st, missing, None)
        assert lib.lib.espm_mu_step_h(C.byref(st), 0, 1, None) == lib.EINVAL, missing
        assert b"ell_hv_n" in lib.lib.espm_mu_last_error(), missing
    # counts that do not fit together, another H rule
    keep += _fake_ptrs(st, hv_ptrs)
    for n_, npx, ngrp, rule in ((4, 5, 3, 0), (4, 2, 5, 0), (4, 0, 3, 0), (-1, 0, 0, 0), (4, 2, 3, 1)):
        st.ell_hv_n, st.ell_hv_npx, st.ell_hv_ngrp, st.h_rule = n_, npx, ngrp, rule
        assert lib.lib.espm_mu_step_h(C.byref(st), 0, 1, None) == lib.EINVAL, (n_, npx, ngrp, rule)
        assert b"ell_hv_n" in lib.lib.espm_mu_last_error()
    # the builder's entry points check their arguments before they launch
    st.ell_hv_n, st.h_rule = 0, 0
    assert lib.lib.espm_mu_ell_heavy_count(C.byref(st), None, lib.SRC_F32, lib.LAYOUT_CM, 1000, None, None, None, None) == lib.EINVAL
    assert lib.lib.espm_mu_ell_heavy_fill(C.byref(st), C.addressof(keep[0]), 7, lib.LAYOUT_CM, 1000, C.addressof(keep[1]), C.addressof(keep[2]), None) == lib.EINVAL
    assert lib.lib.espm_mu_ell_heavy_fill(C.byref(st), C.addressof(keep[0]), lib.SRC_F32, lib.LAYOUT_PM, 10, C.addressof(keep[1]), C.addressof(keep[2]), None) == lib.EINVAL
    del keep
