"""Streamed lists of the sparse store with a part of them kept in the last-level cache (include/espm_mu.h: ell_keep_h, ell_keep_w): the
fused kernel's streamed instance reads the kept list groups / channel groups with plain loads and the others with non-temporal ones -
the same rows in the same order, so W, H and the losses are the same BITS at every setting.

The full geometry on two blocks (160 channels = 3 channel groups, 32 x 64 pixels, tile_px = 512: 8 list groups per tile), the fused
launch forced, ESPM_ELL_STREAM_MB=0 so that the streamed instance runs although these lists would fit any cache.  Of the 4 iterations
the first launch is the generic instance (no previous H), the others the lean, streamed one.  k = 3, 5, 6, 8: the walk with two register
sets, the implicit fifth component, the ring walk, the halved batches."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, NX, NY, TILE, ITERS = 160, 32, 64, 512, 4
GROUPS_H, GROUPS_W = TILE // 64, (N + 63) // 64
# (ell_keep_h, ell_keep_w): everything kept, the H walk only, the W walk only, a mixed setting; compared with nothing kept
SETTINGS = [(GROUPS_H, GROUPS_W), (GROUPS_H, 0), (0, GROUPS_W), (3, 2)]
KW = dict(simplex_H=True, simplex_W=False, lambda_L=1.0)

_cache = {}


def _problem(k):
    if k not in _cache:
        rng = np.random.default_rng(7000 + k)
        p = NX * NY
        Ht = rng.random((k, p)) ** 2 + 0.03
        Ht /= Ht.sum(axis=0, keepdims=True)
        Wt = rng.random((N, k)) ** 3 + 0.02
        Wt *= 0.25 / (Wt @ Ht).mean()
        X = rng.poisson(Wt @ Ht).astype(np.float64)   # mean 0.25: ones, larger counts and padding all occur in the lists
        X[X.sum(axis=1) == 0, 0] = 1.0
        X[0, X.sum(axis=0) == 0] = 1.0
        W0 = (rng.random((N, k)) * Wt.mean() * 2 + 1e-3).astype(np.float32)
        H0 = rng.random((k, p)) + 0.05
        H0 = (H0 / H0.sum(axis=0, keepdims=True)).astype(np.float32)
        _cache[k] = (X, W0, H0)
    return _cache[k]


def _engine(k, monkeypatch, stream=True):
    from espm_amd.engine import MUEngine
    monkeypatch.setenv("ESPM_ELL_STREAM_MB", "0" if stream else "1000000")
    monkeypatch.delenv("ESPM_ELL_KEEP_GROUPS", raising=False)
    monkeypatch.delenv("ESPM_ELL_KEEP_MB", raising=False)
    X, W0, H0 = _problem(k)
    eng = MUEngine(X, k, shape_2d=(NX, NY), x_store="ell", tile_px=TILE, fused="always", tol=0.0, max_iter=ITERS + 2, **KW)
    assert eng.x_store == "ell" and eng.st.tile_px == TILE and eng.st.ell_pb == 2 * TILE and eng.st.nblk_w == 2 and eng.st.n_cg == GROUPS_W
    assert eng.lib.espm_mu_fused_applies(ctypes.byref(eng.st)) == 1 and eng.st.ell_stream == int(stream)
    return eng, W0, H0


def _run(eng, W0, H0, keep_h, keep_w):
    eng.st.ell_keep_h, eng.st.ell_keep_w = keep_h, keep_w
    eng.load_state(W0, H0)
    eng.iterate(ITERS, final_loss=True)
    torch.cuda.synchronize()
    return eng.get_W(), eng.get_H(), np.array(eng.history()["loss"])


@pytest.mark.parametrize("k", [3, 5, 6, 8])
def test_kept_lists_change_no_bit(k, monkeypatch):
    eng, W0, H0 = _engine(k, monkeypatch)
    ref = _run(eng, W0, H0, 0, 0)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and np.isfinite(ref[2]).all() and len(ref[2]) >= ITERS
    assert ref[2][-1] < ref[2][0]
    for keep_h, keep_w in SETTINGS:
        W, H, loss = _run(eng, W0, H0, keep_h, keep_w)
        assert np.array_equal(W, ref[0]) and np.array_equal(H, ref[1]) and np.array_equal(loss, ref[2]), (keep_h, keep_w)


def test_keep_values_out_of_range_are_refused_before_anything_runs(monkeypatch):
    eng, W0, H0 = _engine(5, monkeypatch)
    ref = _run(eng, W0, H0, 0, 0)
    for keep_h, keep_w in [(GROUPS_H + 1, 0), (0, GROUPS_W + 1), (-1, 0), (0, -1)]:
        eng.st.ell_keep_h = eng.st.ell_keep_w = 0
        eng.load_state(W0, H0)
        eng.st.ell_keep_h, eng.st.ell_keep_w = keep_h, keep_w
        with pytest.raises(ValueError, match="ell_keep_h"):
            eng.iterate(1, final_loss=False)
        eng.st.ell_keep_h = eng.st.ell_keep_w = 0
        torch.cuda.synchronize()
        assert eng.st.it == 0 and np.array_equal(eng.get_W(), W0) and np.array_equal(eng.get_H(), H0)   # nothing was enqueued
    out = _run(eng, W0, H0, 1, 1)
    assert np.array_equal(out[0], ref[0]) and np.array_equal(out[2], ref[2])


def test_keep_values_are_ignored_without_ell_stream(monkeypatch):
    eng, W0, H0 = _engine(5, monkeypatch, stream=False)
    ref = _run(eng, W0, H0, 0, 0)
    out = _run(eng, W0, H0, 99, -5)
    assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1]) and np.array_equal(out[2], ref[2])
    # ... and the plain-load launch computes what the streamed one does
    eng2, _, _ = _engine(5, monkeypatch)
    out2 = _run(eng2, W0, H0, GROUPS_H, 1)
    assert np.array_equal(out2[0], ref[0]) and np.array_equal(out2[1], ref[1]) and np.array_equal(out2[2], ref[2])
