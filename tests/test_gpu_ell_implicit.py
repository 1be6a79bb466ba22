"""The fused sparse kernel at k = 5 with its fifth component implicit (csrc/mu_h_kernel.hpp, FixTab: tables of normalised rows, one
16-byte gather per list entry, the last numerator / accumulator restored from the sum of the ratios, the loss corrected by
sum_c cnt[c] log2 sigma_c from espm_mu_state.ell_blk_cnt): one iteration and the loss against the fp64 oracle on both geometries, the
neighbouring component counts, a state built to make the restoring subtractions cancel, edge inputs, the loss bookkeeping over five
iterations, bit-reproducibility, and a two-rank sharded fit.  Everything goes through the C ABI (MUEngine on the sparse store).

The implicit form lives in the fused kernel's LEAN instances (simplex over H, Laplacian, a previous H to compare with, no fill or heavy
numerators); the generic instances keep the explicit tables.  The first launch after load_state has no previous H and is a generic one,
so the tests that look at ONE launch from a prepared state load it as a fit's state at iteration 1 (_load_running)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import mu_oracle as oc

pytestmark = pytest.mark.gpu

# (channels, image rows, image columns, tile_px): the run-time-sized instance on several blocks | the full geometry on two blocks
SHAPES = [(96, 16, 64, 64), (160, 32, 64, 512)]
KW = dict(simplex_H=True, simplex_W=False, lambda_L=1.0)
# loss 1e-5 relative, H 5e-5 absolute, W 2e-4 of its scale
LOSS_RTOL, H_ATOL, W_TOL = 1e-5, 5e-5, 2e-4

_cache = {}


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _problem(n, nx, ny, k, kind="random"):
    """Poisson counts of mean 0.25 (ones, larger counts and padding all occur in the lists) and a start state, rounded to fp32 so that
    the oracle and the device start from the same numbers.  kind = "cancel": the last component holds >= 0.998 of every pixel of H0
    and the last column of W0 is 1e3 x the others on a tenth of the channels."""
    key = (n, nx, ny, k, kind)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(1000 * n + 10 * k + nx)
    p = nx * ny
    Ht = rng.random((k, p)) ** 2 + 0.03
    Ht /= Ht.sum(axis=0, keepdims=True)
    Wt = rng.random((n, k)) ** 3 + 0.02
    Wt *= 0.25 / (Wt @ Ht).mean()
    X = rng.poisson(Wt @ Ht).astype(np.float64)
    X[X.sum(axis=1) == 0, 0] = 1.0
    X[0, X.sum(axis=0) == 0] = 1.0
    W0 = rng.random((n, k)) * Wt.mean() * 2 + 1e-3
    H0 = rng.random((k, p)) + 0.05
    if kind == "cancel":
        H0[:k - 1] *= 0.002 / H0[:k - 1].sum(axis=0, keepdims=True) * rng.random(p)   # the first k - 1 share at most 0.002
        H0[k - 1] = 1.0 - H0[:k - 1].sum(axis=0)
        W0[::10, k - 1] = 1e3 * W0[::10, :k - 1].mean(axis=1)
    else:
        H0 /= H0.sum(axis=0, keepdims=True)
    out = (X, _f32(W0), _f32(H0))
    _cache[key] = out
    return out


def _oracle(X, k, W0, H0, shape, iters, tag):
    key = ("oracle", tag, iters)
    if key not in _cache:
        n = X.shape[0]
        ref = oc.fit(X, k, W=W0.copy(), H=H0.copy(), shape_2d=shape, tol=0, no_stop_criterion=True, max_iter=iters, exact_root=True, **KW)
        L = oc.laplacian_matrix(*shape)
        loss0 = oc.smooth_nmf_loss(oc.remove_zeros_lines(X, oc.LOG_SHIFT), np.eye(n), W0, H0, L, 0, 1, KW["lambda_L"])[0]
        _cache[key] = (ref, loss0)
    return _cache[key]


def _engine(X, k, shape, tile, iters, **extra):
    from espm_amd.engine import MUEngine
    eng = MUEngine(X, k, shape_2d=shape, x_store="ell", tile_px=tile, fused="always", tol=0.0, max_iter=iters + 2, **KW, **extra)
    assert eng.x_store == "ell" and eng.st.tile_px == tile and eng.lib.espm_mu_fused_applies(ctypes.byref(eng.st)) == 1
    return eng


def _load_running(eng, W0, H0):
    """(W0, H0) as the state of a fit that is under way: a previous H exists (equal to H0: rel_H = 0), the history continues at slot 1 -
    the next launch is then the lean instance, as every launch of a fit after its first."""
    eng.load_state(W0, H0)
    eng.h[1].copy_(eng.h[0])
    eng.st.it = 1


def _assert_lean_implicit(eng, W0, H0):
    """The launch that follows _load_running IS the lean instance with the implicit tables: only that one needs ell_blk_cnt, and the
    launcher refuses it without (ESPM_EINVAL before anything is enqueued); a generic, explicit launch would simply run."""
    _load_running(eng, W0, H0)
    keep = eng.st.ell_blk_cnt
    eng.st.ell_blk_cnt = None
    try:
        with pytest.raises(Exception, match="ell_blk_cnt"):
            eng.iterate(1, final_loss=False)
    finally:
        eng.st.ell_blk_cnt = keep


def _check_one_iteration(X, k, W0, H0, shape, tile, tag):
    """One iteration (W', H') and the losses of the initial state and of the state after it - both from the fused launch's H walk -
    against the oracle."""
    ref, loss0 = _oracle(X, k, W0, H0, shape, 1, tag)
    eng = _engine(X, k, shape, tile, 3)
    if k == 5:
        _assert_lean_implicit(eng, W0, H0)
    _load_running(eng, W0, H0)
    eng.iterate(1, final_loss=False)
    torch.cuda.synchronize()
    W, H = eng.get_W(), eng.get_H()
    eng.iterate(1, final_loss=False)     # (its H walk evaluates the state after the first iteration)
    torch.cuda.synchronize()
    loss = eng.history(upto=2)["loss"][1:]
    dl0, dl1 = abs(loss[0] - loss0) / abs(loss0), abs(loss[1] - ref["losses"][0]) / abs(ref["losses"][0])
    dH = np.abs(H - ref["H"]).max()
    dW = np.abs(W - ref["W"]).max() / np.abs(ref["W"]).mean()
    print(f"{tag}: loss {dl0:.2e} {dl1:.2e}  max|dH| {dH:.2e}  max|dW| / mean W {dW:.2e}")
    assert np.isfinite(W).all() and np.isfinite(H).all() and np.isfinite(loss).all()
    assert dl0 < LOSS_RTOL and dl1 < LOSS_RTOL
    np.testing.assert_allclose(H, ref["H"], rtol=0, atol=H_ATOL)
    np.testing.assert_allclose(W, ref["W"], rtol=W_TOL, atol=W_TOL * np.abs(ref["W"]).mean())


@pytest.mark.parametrize("k", [5, 4, 6])
@pytest.mark.parametrize("shape", SHAPES, ids=["small_geometry", "full_geometry"])
def test_one_iteration_against_the_oracle(shape, k):
    n, nx, ny, tile = shape
    X, W0, H0 = _problem(n, nx, ny, k)
    assert (X == 1).sum() > 0.1 * X.size and (X > 1).sum() > 0.01 * X.size
    _check_one_iteration(X, k, W0, H0, (nx, ny), tile, f"random n={n} tile={tile} k={k}")


@pytest.mark.parametrize("shape", SHAPES, ids=["small_geometry", "full_geometry"])
def test_cancellation_case(shape):
    """The last component holds >= 0.998 of every pixel, so y' = h_4 + sum g'_k (h_k - h_4) and num_4 = S - (num_0 + .. + num_3)
    cancel as far as they can; W's last column is 1e3 x the others on a tenth of the channels, so their normalised rows are ~1e-3.
    (On the CPU the oracle is finite on these inputs, and when every input moves by one fp32 ulp its W' moves by at most 2.0e-6
    of mean W, its H' by 1.5e-7 and its loss by 5e-10 relative: two orders inside the bounds, which the inputs' own conditioning
    therefore does not use up.)"""
    n, nx, ny, tile = shape
    X, W0, H0 = _problem(n, nx, ny, 5, "cancel")
    assert H0[4].min() >= 0.998
    _check_one_iteration(X, 5, W0, H0, (nx, ny), tile, f"cancel n={n} tile={tile}")


@pytest.mark.parametrize("lean", [True, False], ids=["lean_instance", "generic_instance"])
@pytest.mark.parametrize("shape", SHAPES, ids=["small_geometry", "full_geometry"])
def test_edge_inputs(shape, lean):
    """A pixel without counts (its numerator is the fill's), a channel without counts, a heavy element (count 300: outside the lists
    and outside ell_blk_cnt) and entries of W at the floor.  (Fill and heavy numerators select the generic instance, which keeps the
    explicit tables: what that case pins is the store - ell_blk_cnt without the heavy element - and that such images still fit; the
    lean case keeps the channel without counts and the floor entries, which the implicit tables do see.)"""
    n, nx, ny, tile = shape
    X, W0, H0 = (a.copy() for a in _problem(n, nx, ny, 5))
    X[3, :] = 0
    if not lean:
        X[:, 7] = 0
        X[10, 20] = 300
    W0[5, :] = oc.LOG_SHIFT
    W0[::7, 4] = oc.LOG_SHIFT
    W0[::9, 1] = oc.LOG_SHIFT
    W0 = _f32(W0)
    iters = 3
    ref = oc.fit(X, 5, W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), tol=0, no_stop_criterion=True, max_iter=iters, exact_root=True, **KW)
    eng = _engine(X, 5, (nx, ny), tile, iters)
    assert (eng.st.ell_hv_n, eng.st.ell_fill_n) == ((0, 0) if lean else (1, 1))
    cnt = eng.ell["blk_cnt"].cpu().numpy()
    assert cnt.shape == (eng.st.nblk_w, eng.st.n_pad) and cnt.sum() == X.sum() - (0 if lean else 300) and cnt[:, 3].sum() == 0
    if lean:
        _assert_lean_implicit(eng, W0, H0)
    eng.load_state(W0, H0)
    eng.iterate(iters, final_loss=True)
    torch.cuda.synchronize()
    W, H, loss = eng.get_W(), eng.get_H(), eng.history()["loss"]
    assert np.isfinite(W).all() and np.isfinite(H).all() and np.isfinite(loss).all()
    dl = np.abs(loss[1:] - ref["losses"]) / np.abs(ref["losses"])
    print(f"edge n={n} tile={tile}: loss {dl.max():.2e}  max|dH| {np.abs(H - ref['H']).max():.2e}  "
          f"max|dW| / mean W {np.abs(W - ref['W']).max() / np.abs(ref['W']).mean():.2e}")
    assert dl.max() < LOSS_RTOL
    np.testing.assert_allclose(H, ref["H"], rtol=0, atol=H_ATOL)
    np.testing.assert_allclose(W, ref["W"], rtol=W_TOL, atol=W_TOL * np.abs(ref["W"]).mean())


@pytest.mark.parametrize("shape", SHAPES, ids=["small_geometry", "full_geometry"])
def test_loss_bookkeeping_over_five_iterations(shape):
    """The history of the fused launches (normalised tables, corrected per block) against SmoothNMF.loss in fp64 on the states the
    device returned, 1e-6 relative: states 0 .. 5, each evaluated by the H walk of the launch that updates it."""
    n, nx, ny, tile = shape
    X, W0, H0 = _problem(n, nx, ny, 5)
    eng = _engine(X, 5, (nx, ny), tile, 8)
    _assert_lean_implicit(eng, W0, H0)
    states = [(W0, H0)]
    for it in range(1, 6):                      # (bit-reproducible: the state after `it` iterations of any run)
        eng.load_state(W0, H0)
        eng.iterate(it, final_loss=False)
        torch.cuda.synchronize()
        states.append((eng.get_W().astype(np.float64), eng.get_H().astype(np.float64)))
    eng.load_state(W0, H0)
    eng.iterate(6, final_loss=False)
    torch.cuda.synchronize()
    loss = eng.history(upto=5)["loss"]
    L = oc.laplacian_matrix(nx, ny)
    want = np.array([oc.smooth_nmf_loss(X, np.eye(n), W, H, L, 0, 1, KW["lambda_L"])[0] for W, H in states])
    rel = np.abs(loss - want) / np.abs(want)
    print(f"bookkeeping n={n} tile={tile}: {rel}")
    assert rel.max() < 1e-6


@pytest.mark.parametrize("shape", SHAPES, ids=["small_geometry", "full_geometry"])
def test_two_engines_give_the_same_bits_over_20_launches(shape):
    n, nx, ny, tile = shape
    X, W0, H0 = _problem(n, nx, ny, 5)
    out = []
    for _ in range(2):
        eng = _engine(X, 5, (nx, ny), tile, 20)
        _assert_lean_implicit(eng, W0, H0)
        eng.load_state(W0, H0)
        eng.iterate(20, final_loss=True)
        torch.cuda.synchronize()
        out.append((eng.get_W(), eng.get_H(), eng.history()["loss"]))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_two_rank_shards_agree_on_w(monkeypatch):
    """Two ranks (threads, tests/thread_ranks.py) with a 16-row shard each: W bit-identical on both, and the fit that of the one-GPU
    oracle."""
    from thread_ranks import run_ranks
    monkeypatch.setenv("ESPM_XCHG", "collective")
    n, nx, ny, tile = 96, 32, 64, 64
    X, W0, H0 = _problem(n, nx, ny, 5)
    iters = 4

    def body(group, rank):
        from espm_amd import sharding
        from espm_amd.engine import MUEngine
        row0, rows = sharding.split_rows(nx, 2, rank)
        sl = slice(row0 * ny, (row0 + rows) * ny)
        eng = MUEngine(np.ascontiguousarray(X[:, sl]), 5, shape_2d=(rows, ny), x_store="ell", tile_px=tile, fused="always", tol=0.0,
                       max_iter=iters + 2, group=group, device="cuda:0", **KW)
        fused = eng.lib.espm_mu_fused_applies(ctypes.byref(eng.st))
        eng.load_state(W0, H0[:, sl])
        eng.iterate(iters, final_loss=True)
        torch.cuda.synchronize()
        return dict(W=eng.get_W(), H=eng.get_H(), loss=eng.history()["loss"], fused=fused)

    res = run_ranks(2, body)
    assert res[0]["fused"] == 1 and res[1]["fused"] == 1
    assert np.array_equal(res[0]["W"], res[1]["W"]) and np.array_equal(res[0]["loss"], res[1]["loss"])
    ref = oc.fit(X, 5, W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), tol=0, no_stop_criterion=True, max_iter=iters, exact_root=True, **KW)
    H = np.concatenate([res[0]["H"], res[1]["H"]], axis=1)
    dl = np.abs(res[0]["loss"][1:] - ref["losses"]) / np.abs(ref["losses"])
    print(f"sharded: loss {dl.max():.2e}  max|dH| {np.abs(H - ref['H']).max():.2e}")
    assert dl.max() < LOSS_RTOL
    np.testing.assert_allclose(H, ref["H"], rtol=0, atol=H_ATOL)
    np.testing.assert_allclose(res[0]["W"], ref["W"], rtol=W_TOL, atol=W_TOL * np.abs(ref["W"]).mean())
