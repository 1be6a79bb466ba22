"""The dense stores at the tile and block sizes large images get ("geometry of the dense stores"), on images of a
few hundred pixels, against the fp64 oracle.  The table is tests/dense_geometry_cases.py; tests/test_dense_geometry_cpu.py holds its
`expect` column to the loops' arithmetic without a GPU.

Per row: (1) the engine's own state must have the row's geometry - store, tile_px, x_tile, nblk_w, the build, no_fused: a row that lands
elsewhere fails; (2) one H step against the oracle's step on the same state (exact root for the default rule); (3) where the row says
so, one W step against oc.multiplicative_step_w and - vector W accumulation - the reduced numerator eng.a against (X / (GW H)) H^T in
fp64 from the fp32 inputs; (4) where the row says so, three iterations against oc.fit; (5) rows on the matrix cores run again with
fused=False from the same state and must agree with that vector twin.  W0, H0 and the fp32 store's X are rounded to fp32 before either
side sees them.

Tolerances.  One H step, vector kernels: F32 of tests/test_gpu_updates.py (rtol 2e-5, atol 2e-6) without the simplex over H, rtol 3e-5 /
atol 3e-6 with it.  One W step: rtol 3e-5, atol 1e-7 (test_step_w_golden).  Three iterations: loss rtol 1e-5, H rtol 2e-4 / atol 2e-5,
W rtol 2e-4 / atol 2e-4 mean |W|, bad == 0 (test_count_stores_match_oracle, _wide_build_against_oracle).  Matrix-core rows: their one
H step against the oracle at the three-iteration bound for H (what the project holds those kernels to against the oracle), and
against the vector twin max |dH| < 2e-5 and max |dW| / (|W| + 1e-6 mean |W|) < 2e-4 after every step the row runs
(test_matrix_core_kernels_of_the_wide_build_at_full_size: the project's figures for the bf16 hi / lo split).  With 17..32 components
the 8-bit and bf16 stores have no vector kernels: the twin of such a row runs the same image - exact in fp32 - on the fp32 store.

The numerator.  A[kk, c] = sum_j X[c, j] / Y[c, j] * H[kk, j] with Y[c, j] = sum_kk GW[c, kk] H[kk, j]; every term is non-negative, so
the relative error is bounded by the roundings on the way, u = 2^-24 each: k for Y (one product, k - 1 fused multiply-adds), 2 for
the hardware reciprocal (1 ulp), 1 for X times it, ppb for the block's sum (one fused multiply-add per pixel, its product unrounded),
nblk_w for the sum over the blocks: N = k + 3 + ppb + nblk_w, rtol = N u / (1 - N u) - 4.4e-6 at most over the table
(k = 12, ppb = 49, nblk_w = 9 gives 4.4e-6; the 16-pixel blocks of the H256 rows, k = 8 and 28 blocks, 3.3e-6).

Every row prints one `DENSE-GEOM` line with its geometry and, per check, its worst error over the bound (run with -s).  On an MI355X
no check of any row is above 0.12 of its bound (the loss of an Hmfma-trips row), the numerator at most 0.063, the matrix cores
against their vector twin at most 0.019: a group dropped, taken twice or from the wrong ring slot is a first-order error, thousands
of times the bound."""
import functools
import time
import zlib

import numpy as np
import pytest

import dense_geometry_cases as dg
from oracle import mu_oracle as oc
from test_gpu_updates import F32

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
TOL = 1e-4
U = 2.0 ** -24
H_SIMPLEX = dict(rtol=3e-5, atol=3e-6)
H_FIT = dict(rtol=2e-4, atol=2e-5)
TWIN_DH, TWIN_DW = 2e-5, 2e-4


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=4)
def _problem(row_id):
    """Poisson counts of a random model for the row (u8: clipped to 255; bf16: half-integers below 2^7; f32: counts times a random
    factor), a start (W0, H0) and the oracle's results, computed once per row.  Seeded by the row's id."""
    row = next(r for r in dg.CASES if r["id"] == row_id)
    k, n, m, opt, (nx, ny) = row["k"], row["n"], row["m"], row["opt"], row["shape"]
    rng = np.random.default_rng(zlib.crc32(row_id.encode()))
    p, M = nx * ny, (m if m else n)
    H = rng.random((k, p)) ** 2 + 0.03
    W = rng.random((M, k)) + (0.1 if m else 0.2)
    G = rng.random((n, m)) * (rng.random((n, m)) < 0.5) + 0.01 if m else None
    W0 = (0.5 + rng.random((M, k))) * W.mean()
    H0 = rng.random((k, p)) + 0.05
    if opt["simplex_W"]:   # W on the simplex, the counts' scale on H
        W, W0 = W / W.sum(axis=0), W0 / W0.sum(axis=0)
    else:
        H, H0 = H / H.sum(axis=0), H0 / H0.sum(axis=0)
    Y = (G @ W if m else W) @ H
    s = 4.0 / Y.mean()   # four counts per entry: no channel and no pixel without counts
    if opt["simplex_W"]:
        H0 = H0 * s * H.mean() / H0.mean()
    else:
        W0 = W0 * s
    counts = np.minimum(rng.poisson(Y * s), 255).astype(np.float64)
    X = {"u8": counts, "bf16": counts / 2, "f32": _f32(counts * (0.5 + rng.random(counts.shape)))}[row["store"]]
    assert (X.sum(axis=1) > 0).all() and (X.sum(axis=0) > 0).all()
    if G is not None:
        G = _f32(G)
    W0, H0 = _f32(W0), _f32(H0)
    Gd = G if m else np.eye(n)
    L = oc.laplacian_matrix(nx, ny)
    kw = dict(simplex_H=opt["simplex_H"], simplex_W=opt["simplex_W"], lambda_L=opt["lambda_L"], mu=opt["mu"])
    pr = dict(row=row, X=X, G=G, Gd=Gd, W0=W0, H0=H0, kw=kw, p=p, gamma=None)
    rule = row["rule"]
    if rule == "kl":
        pr["h_ref"] = oc.multiplicative_step_h(X, Gd, W0, H0, simplex_H=kw["simplex_H"], mu=kw["mu"], lambda_L=kw["lambda_L"], L=L, exact_root=True)
    elif rule == "l2":
        pr["h_ref"] = oc.multiplicative_step_h(X, Gd, W0, H0, simplex_H=False, l2=True)
    elif rule == "hq":
        pr["h_ref"] = oc.multiplicative_step_hq(X, Gd, W0, H0, simplex_H=False, lambda_L=kw["lambda_L"], L=L)
    else:   # projected gradient: step sizes as tests/test_gpu_fuzz.py draws them
        gh = np.abs(oc.gradH(X, Gd, W0, H0, mu=kw["mu"], lambda_L=kw["lambda_L"], L=L)).max()
        gw = np.abs(oc.gradW(X, Gd, W0, H0)).max()
        pr["gamma"] = [float(gh / 0.05), float(gw / (0.2 * W0.mean()))]
        pr["h_ref"] = oc.proj_grad_step_h(X, Gd, W0, H0, pr["gamma"][0], simplex_H=False, mu=kw["mu"], lambda_L=kw["lambda_L"], L=L)
    if row["w_step"]:
        pr["w_ref"] = oc.multiplicative_step_w(X, Gd, W0, H0, simplex_W=kw["simplex_W"])
    if row["fit"]:
        pr["fit_ref"] = oc.fit(X, k, G=G, W=W0.copy(), H=H0.copy(), shape_2d=(nx, ny), exact_root=True, no_stop_criterion=True, max_iter=3,
                               tol=TOL, **kw)
    return pr


def _engine(pr, fused, store=None):
    from espm_amd.engine import MUEngine
    row = pr["row"]
    extra = {}
    if row["rule"] == "l2":
        extra = dict(compute_loss=False)          # (the Frobenius H step has no loss pieces: updates.py:109-118)
    elif row["rule"] == "hq":
        extra = dict(h_rule=1)
    elif row["rule"] == "pg":
        extra = dict(h_rule=2, sigmaL=pr["gamma"][0], pg_gamma_w=pr["gamma"][1])
    return MUEngine(pr["X"], row["k"], G=pr["G"], shape_2d=row["shape"], max_iter=6, tol=TOL, x_store=store or row["store"],
                    tile_px=row["tile_px"], x_tile=row["x_tile"], w_blocks=row["w_blocks"], fused=fused, **extra, **pr["kw"])


def _assert_geometry(eng, row, fused, store):
    p = row["shape"][0] * row["shape"][1]
    nblk = dg.w_geometry(p, row["w_blocks"])[1] if row["w_blocks"] else dg.default_w_blocks(p)
    got = (eng.x_store, int(eng.st.tile_px), int(eng.st.x_tile), int(eng.st.nblk_w), eng.V.KP, int(eng.st.no_fused))
    want = (store, row["tile_px"], row["x_tile"] or row["tile_px"], nblk, dg.build_of(row["k"]), 0 if fused else 1)
    assert got == want, f"{row['id']}: (store, tile_px, x_tile, nblk_w, KP, no_fused) is {got}, the row needs {want}"
    assert tuple(eng.a_slab.shape) == (nblk, row["k"], int(eng.st.n_pad)) and int(eng.st.n_pad) == dg.n_pad_of(row["n"])
    assert tuple(eng.x_cm.shape)[0] == int(eng.st.p_pad) // (row["x_tile"] or row["tile_px"])
    return nblk


def _worst(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|): at most 1 where assert_allclose passes."""
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref))))


def _numerator_ref(eng, pr):
    """(X / (GW H)) H^T in fp64 from the fp32 inputs as the device holds them: the rows of G W, H and the pixel-major X."""
    k, n, p = pr["row"]["k"], pr["row"]["n"], pr["p"]
    gw = eng.gw_s[:n, :k].double().cpu().numpy()
    H = eng.h[eng.st.cur][:, :p].double().cpu().numpy()
    X = eng.x_pm[:, :n].double().cpu().numpy()          # (p, n)
    return ((X.T / (gw @ H)) @ H.T).T                    # (k, n)


def _run_engine(pr, fused, store, against_oracle):
    """Steps 1-4 on one engine; returns (figures, the arrays the twin comparison needs)."""
    import torch
    row = pr["row"]
    k, n = row["k"], row["n"]
    eng = _engine(pr, fused, store)
    nblk = _assert_geometry(eng, row, fused, store)
    fig, out = {}, {}
    mfma_h = fused and dg.h_on_matrix_cores(row)
    # 2. one H step
    eng.load_state(pr["W0"], pr["H0"])
    Hn = eng.step_h_only(l2=row["rule"] == "l2").astype(np.float64)
    out["H1"] = Hn
    tol = H_FIT if mfma_h else (H_SIMPLEX if pr["kw"]["simplex_H"] else F32)
    fig["H1"] = _worst(Hn, pr["h_ref"], **tol)
    checks = [lambda: np.testing.assert_allclose(Hn, pr["h_ref"], err_msg=row["id"] + ": one H step", **tol)]
    # 3. one W step
    if row["w_step"]:
        eng.load_state(pr["W0"], pr["H0"])
        vector_w = not (fused and dg.w_on_matrix_cores(row))
        a_ref = _numerator_ref(eng, pr) if vector_w else None
        Wn = eng.step_w_only().astype(np.float64)
        out["W1"] = Wn
        fig["W1"] = _worst(Wn, pr["w_ref"], 3e-5, 1e-7)
        checks.append(lambda: np.testing.assert_allclose(Wn, pr["w_ref"], rtol=3e-5, atol=1e-7, err_msg=row["id"] + ": one W step"))
        if vector_w:
            N = k + 3 + -(-pr["p"] // nblk) + nblk
            rtol = N * U / (1 - N * U)
            a = eng.a[:k, :n].double().cpu().numpy()
            fig["A"] = _worst(a, a_ref, rtol, 1e-30)
            checks.append(lambda: np.testing.assert_allclose(a, a_ref, rtol=rtol, atol=1e-30, err_msg=row["id"] + ": reduced numerator"))
    # 4. three iterations
    if row["fit"]:
        ref = pr["fit_ref"]
        eng.load_state(pr["W0"], pr["H0"])
        eng.iterate(3, final_loss=True)
        torch.cuda.synchronize()
        h = eng.history()
        We, He = eng.get_W().astype(np.float64), eng.get_H().astype(np.float64)
        out["H3"], out["W3"] = He, We
        if not pr["kw"]["simplex_H"] and not pr["kw"]["simplex_W"]:
            We, He = oc.rescaled_DH(We, He)   # base.py:399-400: what the fit loop returns without a simplex
        wa = 2e-4 * np.abs(ref["W"]).mean()
        fig.update(loss=_worst(h["loss"][1:], ref["losses"], LOSS_RTOL, 0.0), H3=_worst(He, ref["H"], **H_FIT), W3=_worst(We, ref["W"], 2e-4, wa),
                   bad=float(h["bad"].sum()))
        checks += [lambda: np.testing.assert_allclose(h["loss"][1:], ref["losses"], rtol=LOSS_RTOL, err_msg=row["id"] + ": losses"),
                   lambda: np.testing.assert_allclose(He, ref["H"], err_msg=row["id"] + ": H after three iterations", **H_FIT),
                   lambda: np.testing.assert_allclose(We, ref["W"], rtol=2e-4, atol=wa, err_msg=row["id"] + ": W after three iterations"),
                   lambda: np.testing.assert_equal(h["bad"].sum(), 0)]
    return fig, out, (checks if against_oracle else [])


def _twin_figures(mf, vt):
    """max |dH| over 2e-5 and the relative dW of test_matrix_core_kernels_of_the_wide_build_at_full_size over 2e-4, per step both ran."""
    fig = {}
    for key in ("H1", "H3"):
        if key in mf:
            fig["d" + key] = float(np.abs(mf[key] - vt[key]).max()) / TWIN_DH
    for key in ("W1", "W3"):
        if key in mf:
            fig["d" + key] = float((np.abs(mf[key] - vt[key]) / (np.abs(vt[key]) + 1e-6 * np.abs(vt[key]).mean())).max()) / TWIN_DW
    return fig


def _line(tag, fig):
    return f"    {tag}: " + " ".join(f"{key} {v:.3f}" for key, v in fig.items()) + " (of 1)"


@pytest.mark.parametrize("row", dg.CASES, ids=[r["id"] for r in dg.CASES])
def test_dense_geometry(row):
    t0 = time.perf_counter()
    pr = _problem(row["id"])
    fig, out, checks = _run_engine(pr, row["fused"], row["store"], True)
    e = row["expect"]
    print(f"\nDENSE-GEOM {row['id']}: {row['family']} k={row['k']} {row['store']} tile={row['tile_px']} x_tile={row['x_tile'] or row['tile_px']} n={row['n']} "
          f"px={row['shape'][0]}x{row['shape'][1]} m={row['m']} w_blocks={row['w_blocks']} fused={row['fused']} rule={row['rule']} "
          f"-> {e['loop']} {e.get('shapes') or e.get('trips') or e.get('blocks')}")
    print(_line("against the oracle", fig))
    twin = None
    if dg.matrix_core_row(row):
        # 5. the vector twin from the same state (17..32 components off the fp32 store: the same image on the fp32 store)
        store = row["store"] if row["k"] <= 16 else "f32"
        vfig, vout, vchecks = _run_engine(pr, False, store, True)
        twin = _twin_figures(out, vout)
        print(_line(f"vector twin ({store}) against the oracle", vfig))
        print(_line("matrix cores against the vector twin", twin))
        for c in vchecks:   # (the yardstick first: a twin that misses the oracle says nothing about the matrix-core kernels)
            c()
    print(f"    {time.perf_counter() - t0:.2f} s")
    for c in checks:
        c()
    if twin is not None:
        assert all(v < 1.0 for v in twin.values()), f"{row['id']}: matrix cores against the vector twin, over (2e-5, 2e-4): {twin}"


def test_w_blocks_is_refused_where_it_does_not_apply():
    """MUEngine(w_blocks=): 1..ceil(p / 16) on a dense store; the sparse store's blocks are fixed by ell_pb."""
    from espm_amd.engine import MUEngine
    pr = _problem("wring-u8-k5-b10")
    kw = dict(shape_2d=(19, 23), max_iter=2, **pr["kw"])
    for bad in (0, -3, 29):
        with pytest.raises(ValueError, match="w_blocks"):
            MUEngine(pr["X"], 5, G=pr["G"], x_store="u8", w_blocks=bad, **kw)
    with pytest.raises(ValueError, match="w_blocks"):
        MUEngine(pr["X"], 5, G=pr["G"], x_store="ell", w_blocks=4, **kw)
    eng = MUEngine(pr["X"], 5, G=pr["G"], x_store="u8", w_blocks=28, **kw)
    dflt = MUEngine(pr["X"], 5, G=pr["G"], x_store="u8", **kw)
    assert int(eng.st.nblk_w) == int(dflt.st.nblk_w) == 28 and tuple(eng.a_slab.shape) == tuple(dflt.a_slab.shape)


@pytest.mark.parametrize("k", [5, 12])
@pytest.mark.parametrize("store", ["u8", "f32"])
def test_chained_h_step_at_256_pixel_tiles_and_344_channels(store, k):
    """The chained kernel's 256-pixel instance and a channel range of 344 (tests/test_gpu_transform.py reaches it at 128-pixel tiles and
    64 channels): test_chained_general_and_granular_agree_bit_for_bit's comparison through its helper, four H-only iterations."""
    from test_gpu_transform import _child
    chained, general, granular = (_child(store, k, 1.0, mode, n_it=4, geometry=(256, 344, 19, 23)) for mode in ("chained", "general", "granular"))
    assert chained["chain"] == 1 and general["chain"] == 0
    for r in (chained, general, granular):
        assert r["held"] and r["it"] == 4 and r["tile_px"] == 256 and r["store"] == store
    for key in ("h", "hist", "hstat"):
        assert chained[key] == general[key] == granular[key], key
