"""Heavy elements of the sparse count store on the device (include/espm_mu.h, ell_hv_*): integer count images with counts above 255
stay on the sparse store - the HIP builder against the tensor-op one, whole fits against the fp64 oracle, the kernels' forms against
one another and against the dense fp32 store, sharded fits against the single-GPU fit, the store selection and its guards."""
import contextlib
import io
import os
import socket

import numpy as np
import pytest
import torch

from oracle import mu_oracle as oc

pytestmark = pytest.mark.gpu


def _heavy(X, rng, frac=0.005, lo=256, hi=60001):
    """~frac of the elements (at least 3) set to counts in lo .. hi - 1."""
    flat = X.reshape(-1)
    pick = rng.choice(flat.size, size=max(3, int(frac * flat.size)), replace=False)
    flat[pick] = rng.integers(lo, hi, size=pick.size)
    return X


def _problem(n, nx, ny, k, seed, m=None):
    rng = np.random.default_rng(seed)
    p = nx * ny
    H = rng.random((k, p)) ** 2 + 0.03
    H /= H.sum(axis=0, keepdims=True)
    if m:
        G = rng.random((n, m)) * (rng.random((n, m)) < 0.5) + 0.01
        W = rng.random((m, k)) * 30.0 / n
        D = G @ W
    else:
        G, W = None, rng.random((n, k)) ** 3 * 100.0 / n + 1e-3
        D = W
    X = _heavy(rng.poisson(D @ H).astype(np.float64), rng)
    X[5, :] = 0
    X[5, [1, p - 2]] = [700, 256]                 # a channel whose only counts are heavy
    X[:, 9] = 0
    X[[2, n - 1], 9] = [1 << 24, 3000]            # a pixel whose only counts are heavy
    X[X.sum(axis=1) == 0, 0] = 1.0
    X[0, X.sum(axis=0) == 0] = 1.0
    W0 = rng.random(W.shape) * W.mean() * 2 + 1e-3
    H0 = rng.random((k, p)) + 0.05
    H0 /= H0.sum(axis=0, keepdims=True)
    return X, G, W0, H0


# ---- 1. the two builders ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,n,tile,layout,dtype", [(900, 120, 64, "cm", np.float64), (1700, 300, 512, "pm", np.float32),
                                                   (640, 4100, 128, "cm", np.float32), (1100, 200, 256, "pm", np.float64)])
def test_hip_builder_equals_torch_builder(monkeypatch, p, n, tile, layout, dtype):
    from espm_amd.engine import MUEngine
    rng = np.random.default_rng(p + n)
    X = _heavy(rng.poisson(0.4, size=(n, p)).astype(np.float64), rng)
    X[3, 0], X[4, 1] = 256, 1 << 24
    X[X.sum(axis=1) == 0, 0] = 1.0
    X[0, X.sum(axis=0) == 0] = 1.0
    Xin = (X if layout == "cm" else np.ascontiguousarray(X.T)).astype(dtype)
    stores = {}
    for builder in ("hip", "torch"):
        monkeypatch.setenv("ESPM_ELL_BUILDER", builder)
        eng = MUEngine(Xin, 3, layout=layout, x_store="ell", tile_px=tile)
        stores[builder] = (eng.ell, eng.hv_klc.cpu(), eng.st.ell_hv_n)
    (a, ka, na), (b, kb, nb) = stores["hip"], stores["torch"]
    assert na == nb == int((X >= 256).sum())
    for key in ("ell_h_off", "ell_w_off", "chan_perm", "pix_perm"):
        assert torch.equal(a[key].cpu(), b[key].cpu()), key
    # (which ones of a list sit in its unit rows is the builder's choice, tests/test_gpu_updates.py::test_ell_builders_agree): both sets
    # of lists decode to the image without its heavy elements
    from ell_decode import decode
    light = np.ascontiguousarray(np.where(X >= 256, 0, X).T).astype(np.int64)
    for st in (a, b):
        host = {key: (v.cpu() if torch.is_tensor(v) else v) for key, v in st.items() if key != "hv"}
        Xh, Xw, _, _ = decode(host, p, n, eng.st.p_pad, eng.st.ell_cbits, eng.st.tile_px)
        assert np.array_equal(Xh[:p], light) and np.array_equal(Xw[:p], light)
    for key in ("nnz", "entries_h", "entries_w", "rows_h", "rows_w", "n_cg", "nblk_w"):
        assert a[key] == b[key], key
    np.testing.assert_allclose(a["klc"].cpu().numpy(), b["klc"].cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(ka.numpy(), kb.numpy(), rtol=1e-6, atol=1e-6)
    for key in ("n", "npx", "ngrp"):
        assert a["hv"][key] == b["hv"][key], key
    for key in ("px", "px_off", "pm", "grp", "grp_off", "wm"):
        assert torch.equal(a["hv"][key].cpu(), b["hv"][key].cpu()), key
    pm = a["hv"]["pm"].cpu().numpy()
    assert pm[:, 1].min() >= 256 and (pm[:, 1] == 1 << 24).any() and (pm[:, 1] == 256).any()


# ---- 2. whole fits against the oracle ------------------------------------------------------------------------------------------
FITS = [  # (k, G columns or None, keyword arguments)
    (1, None, dict(simplex_H=False, simplex_W=True, lambda_L=0.0)),
    (5, None, dict(simplex_H=True, simplex_W=False, lambda_L=1.0, mu=0.1)),
    (5, 12, dict(simplex_H=True, simplex_W=False, lambda_L=1.0)),
    (8, None, dict(simplex_H=False, simplex_W=True, lambda_L=1.0, mu="vec")),
    (8, 14, dict(simplex_H=False, simplex_W=False, lambda_L=0.0, fixed_H=True)),
    (12, None, dict(simplex_H=True, simplex_W=False, lambda_L=0.0, mu="vec")),
    (16, None, dict(simplex_H=False, simplex_W=True, lambda_L=1.0)),
]


def _fit_case(k, m, kw, seed):
    X, G, W0, H0 = _problem(160, 12, 14, k, seed, m)
    kw = dict(kw)
    if kw.get("mu") == "vec":
        kw["mu"] = np.random.default_rng(seed).random(k) * 0.2
    extra = {}
    if kw.pop("fixed_H", False):
        fH = -np.ones(H0.shape)
        fH[0, ::4] = 0.2
        extra["fixed_H"] = fH
    return X, G, W0, H0, kw, extra


@pytest.mark.parametrize("case", range(len(FITS)))
def test_fit_with_heavy_counts_matches_oracle(case):
    from espm_amd.estimators import SmoothNMF
    k, m, kw0 = FITS[case]
    X, G, W0, H0, kw, extra = _fit_case(k, m, kw0, 40 + case)
    iters = 6
    ref = oc.fit(X, k, G=G, W=W0.copy(), H=H0.copy(), shape_2d=(12, 14), algo="log_surrogate", tol=0, no_stop_criterion=True, max_iter=iters,
                 exact_root=True, **kw, **extra)
    est = SmoothNMF(n_components=k, G=G, shape_2d=(12, 14), algo="log_surrogate", tol=0, no_stop_criterion=True, max_iter=iters, verbose=0,
                    **kw, **extra)
    with contextlib.redirect_stdout(io.StringIO()):
        GW = est.fit_transform(X, W=W0.copy(), H=H0.copy())
    assert est._engine.x_store == "ell" and est._engine.st.ell_hv_n == int((X >= 256).sum())
    np.testing.assert_allclose(est.losses_, ref["losses"], rtol=2e-5)
    np.testing.assert_allclose(est.H_, ref["H"], rtol=5e-4, atol=5e-5)
    np.testing.assert_allclose(GW, ref["GW"], rtol=5e-4, atol=5e-4 * np.abs(ref["GW"]).mean())


# ---- 3. the kernels' forms agree ------------------------------------------------------------------------------------------------
def _engine_run(X, k, iters, shape, W0, H0, **kw):
    from espm_amd.engine import MUEngine
    eng = MUEngine(X, k, shape_2d=shape, max_iter=iters, **kw)
    eng.load_state(W0, H0)
    eng.iterate(iters, final_loss=True)
    torch.cuda.synchronize()
    return eng, eng.get_W(), eng.get_H(), eng.history()["loss"]


def test_two_launches_fused_and_full_geometry_agree(monkeypatch):
    X, _, W0, H0 = _problem(200, 40, 40, 5, 7)
    kw = dict(simplex_H=True, simplex_W=False, lambda_L=1.0, mu=0.1, tol=0.0)
    out = {}
    for name, env in (("two", {"ESPM_FUSED": "0"}), ("fused", {"ESPM_FUSED": "always"}), ("full", {"ESPM_FORCE_ELL_TILE": "512"})):
        with monkeypatch.context() as mp_:
            for key, v in env.items():
                mp_.setenv(key, v)
            eng, W, H, loss = _engine_run(X, 5, 8, (40, 40), W0, H0, **kw)
            assert eng.x_store == "ell" and eng.st.ell_hv_n > 0
            out[name] = (W, H, loss, eng.lib.espm_mu_fused_applies(__import__("ctypes").byref(eng.st)))
    assert out["two"][3] == 0 and out["fused"][3] == 1
    for name in ("fused", "full"):
        np.testing.assert_allclose(out[name][0], out["two"][0], rtol=2e-5, atol=1e-7, err_msg=name)
        np.testing.assert_allclose(out[name][1], out["two"][1], rtol=2e-5, atol=2e-6, err_msg=name)
        np.testing.assert_allclose(out[name][2], out["two"][2], rtol=1e-6, err_msg=name)


# ---- 4. the full geometry against the dense fp32 store ---------------------------------------------------------------------------
def test_full_geometry_against_the_f32_store():
    from espm_amd import synth
    n, nx, ny, k = 2048, 512, 512, 5
    prob = synth.make_problem(n, nx, ny, k, N=60.0, seed=3)
    Xt = synth.sample_torch(prob, "cuda", seed=1000)                      # (p, n) f32 counts
    g = torch.Generator(device="cuda").manual_seed(3)
    nz = torch.nonzero(Xt.view(-1)).flatten()
    pick = nz[torch.randperm(nz.numel(), device="cuda", generator=g)[: nz.numel() // 100]]     # 1 % of the non-zero elements heavy
    Xt.view(-1)[pick] = torch.randint(256, 4001, (pick.numel(),), device="cuda", generator=g).float()
    del nz
    W0, H0 = synth.random_init(n, k, nx * ny, seed=3, scale=60.0 / n)
    kw = dict(layout="pm", simplex_H=True, simplex_W=False, lambda_L=1.0, tol=0.0)
    res = {}
    for store in ("ell", "f32"):
        eng, W, H, loss = _engine_run(Xt, k, 4, (nx, ny), W0, H0, x_store=store, **kw)
        assert eng.x_store == store
        if store == "ell":
            assert eng.st.ell_hv_n == pick.numel() and eng.st.tile_px == 512
        res[store] = (W, H, loss)
        del eng
        torch.cuda.empty_cache()
    np.testing.assert_allclose(res["ell"][0], res["f32"][0], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(res["ell"][1], res["f32"][1], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(res["ell"][2], res["f32"][2], rtol=1e-6)


# ---- 5. sharded -----------------------------------------------------------------------------------------------------------------
SNX, SNY, SK, SITERS = 24, 40, 5, 8


def _shard_data():
    X, _, W0, H0 = _problem(200, SNX, SNY, SK, 13)
    # heavy elements in the boundary image rows of the shards (rows 11, 12 of the 24 split in two; 7, 8 and 15, 16 in three)
    for row in (7, 8, 11, 12, 15, 16):
        X[[4, 50, 120], row * SNY + 3] = [5000, 256, 999]
    return X, W0, H0


SKW = dict(lambda_L=1.0, mu=0.1, simplex_H=True, simplex_W=False, tol=0.0)


def _shard_worker(rank, world, port, out, transport):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), ESPM_XCHG=transport)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from espm_amd import sharding
        from espm_amd.engine import MUEngine
        torch.cuda.set_device(0)
        X, W0, H0 = _shard_data()
        row0, rows = sharding.split_rows(SNX, world, rank)
        sl = slice(row0 * SNY, (row0 + rows) * SNY)
        eng = MUEngine(X[:, sl], SK, shape_2d=(rows, SNY), max_iter=SITERS, group=dist.group.WORLD, device="cuda:0",
                       force_sharded=(world == 1), **SKW)
        eng.load_state(W0, H0[:, sl])
        eng.iterate(SITERS, final_loss=True)
        torch.cuda.synchronize()
        out[rank] = (eng.get_W(), eng.get_H(), eng.history()["loss"], eng.x_store, eng.st.ell_hv_n, eng.exchange.transport)
        eng.exchange.close()
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,transport", [(1, "p2p"), (2, "p2p"), (2, "collective")])
def test_sharded_fit_with_heavy_counts_matches_single_gpu(world, transport):
    import torch.multiprocessing as mp
    X, W0, H0 = _shard_data()
    eng, ref_W, ref_H, ref_loss = _engine_run(X, SK, SITERS, (SNX, SNY), W0, H0, **SKW)
    assert eng.x_store == "ell" and eng.st.ell_hv_n > 0
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_shard_worker, args=(world, _free_port(), out, transport), nprocs=world, join=True)
        res = dict(out)
    assert all(res[r][3] == "ell" and res[r][4] > 0 and res[r][5] == transport for r in range(world))
    H = np.concatenate([res[r][1] for r in range(world)], axis=1)
    np.testing.assert_allclose(res[0][0], ref_W, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(H, ref_H, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(res[0][2], ref_loss, rtol=1e-6)


# ---- 6. selection ---------------------------------------------------------------------------------------------------------------
def test_store_selection(monkeypatch):
    from espm_amd.engine import MUEngine
    X, _, _, _ = _problem(160, 12, 14, 3, 5)
    eng = MUEngine(X, 3)
    assert eng.x_store == "ell" and eng.x_store_note is None
    assert MUEngine(X, 3, x_store="ell").x_store == "ell"
    big = X.copy()
    big[7, 7] = (1 << 24) + 2                     # beyond fp32's exact integers: today's store
    assert MUEngine(big, 3).x_store == "f32"
    with pytest.raises(ValueError):
        MUEngine(big, 3, x_store="ell")
    frac = X + 0.5
    assert MUEngine(frac, 3).x_store in ("bf16", "f32")
    pg = MUEngine(X, 3, h_rule=2)                 # the projected gradient: not wired in
    assert pg.x_store == "f32" and "H rule" in pg.x_store_note
    monkeypatch.setenv("ESPM_ELL_HEAVY", "0")
    off = MUEngine(X, 3)
    assert off.x_store == "f32" and off.x_store_note is None
    with pytest.raises(ValueError):
        MUEngine(X, 3, x_store="ell")


# ---- 7. guards ------------------------------------------------------------------------------------------------------------------
def test_repeated_launches_give_identical_bits():
    from espm_amd.engine import MUEngine
    X, _, W0, H0 = _problem(200, 32, 32, 5, 21)
    eng = MUEngine(X, 5, shape_2d=(32, 32), max_iter=2, simplex_H=True, lambda_L=1.0, mu=0.1)
    assert eng.x_store == "ell" and eng.st.ell_hv_n > 0
    first = None
    for _ in range(200):
        eng.load_state(W0, H0)
        eng.iterate(1, final_loss=True)
        got = (eng.get_W().tobytes(), eng.get_H().tobytes(), eng.history()["loss"].tobytes())
        if first is None:
            first = got
        assert got == first


def test_small_counts_are_untouched_by_the_switch(monkeypatch):
    from espm_amd import synth
    from espm_amd.engine import MUEngine
    prob = synth.make_problem(180, 30, 30, 4, N=20.0, seed=8)
    X = np.minimum(synth.sample_numpy(prob, seed=8), 255.0)
    X[3, 3] = 255
    W0, H0 = synth.random_init(180, 4, 900, seed=8, scale=0.5)
    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("ESPM_ELL_HEAVY", flag)
        eng, W, H, loss = _engine_run(X, 4, 6, (30, 30), W0, H0, simplex_H=True, lambda_L=1.0)
        assert eng.x_store == "ell" and eng.st.ell_hv_n == 0 and "hv" not in eng.ell
        runs.append((W.tobytes(), H.tobytes(), loss.tobytes(), {kk: v.cpu().numpy().tobytes() for kk, v in eng.ell.items() if torch.is_tensor(v)}))
    assert runs[0] == runs[1]
