"""Every form of the W update at the sizes where its dispatch turns ("forms of the W update"), against the fp64
oracle.  The table is tests/w_form_cases.py; tests/test_w_update_form_cpu.py holds its `expect` column to the library's plan
without a GPU.

Per row: (1) the engine's state must take the expected form and kernel instance (`MUEngine.w_update_form()`: the plan the launch
itself switches on) - a row that lands elsewhere fails; (2) one W step (`step_w_only`, the form as espm_mu_w_finish launches it)
against the oracle at the project's one-step tolerance, with the products the next H-step and the stop rule consume - the rows of
G W' / xscale, their column sums, and rel_W of one whole iteration (the form as espm_mu_iterate sequences it: only there do the
local update and the simplex split run) - each recomputed in fp64 from the W' the device returned; (3) three iterations against
oracle.fit.  No predicate of the dispatch depends on the pixel count: the image is 6 x 7 pixels.

Tolerances.  W' of one step: rtol 3e-5, atol 1e-7 (test_step_w_golden).  Rows and column sums of G W' from the returned W': G and W'
are non-negative, so an fp32 dot product of m terms is off by at most (m + 1) 2^-24 relative, the floor and the scale add one
rounding: rtol (m + 2) 2^-24 (m = 1 for G = identity).  rel_W from the returned W' and the fp32 W: a maximum of quotients of fp32
values; a form that evaluates it in fp32 rounds three times (3 x 2^-24 = 1.8e-7), the mean of W' enters times tol = 1e-4: rtol 1e-6.
Three iterations: test_count_stores_match_oracle's and _wide_build_against_oracle's bounds."""
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest

import w_form_cases as wc
from oracle import mu_oracle as oc

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
NX, NY = 6, 7
TOL = 1e-4            # the estimator's tol: the weight of mean(W') in rel_W (base.py:323)
SEEN = {}             # id -> (build, form, detail) of the rows that ran in this process


class _Rows:
    """What oracle.fit needs of a physics model to put a subset of the rows of W under the simplex (espm/models/base.py:217-264)."""

    def __init__(self, G, rows):
        self.G, self.rows = G, rows

    def NMF_update(self, W=None):
        return self.G

    def NMF_simplex(self):
        return self.rows

    def NMF_initialize_W(self, D):
        raise AssertionError("W is given")


def _problem(case):
    """Poisson counts (frac: fractional data) of a random model on the 6 x 7 image, a start (W0, H0) and the row's options as the
    engine and the oracle take them.  Seeded by the row's id."""
    k, n, m, opt = case["k"], case["n"], case["m"], case["opt"]
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()) + opt.get("seed", 0))
    p, M = NX * NY, (m if m else n)
    simplex_W = bool(opt.get("simplex_W"))
    H = rng.random((k, p)) ** 2 + 0.03
    W = rng.random((M, k)) + (0.1 if m else 0.2)
    G = rng.random((n, m)) * (rng.random((n, m)) < 0.5) + 0.01 if m else None
    rows = np.arange(0, M, 2) if opt.get("rows") else None
    W0 = (0.5 + rng.random((M, k))) * W.mean()
    H0 = rng.random((k, p)) + 0.05
    if simplex_W:   # W on the simplex (its subset of rows), the counts' scale on H
        sel = rows if rows is not None else np.arange(M)
        W, W0 = W / W[sel].sum(axis=0), W0 / W0[sel].sum(axis=0)
    else:
        H, H0 = H / H.sum(axis=0), H0 / H0.sum(axis=0)
    Y = (G @ W if m else W) @ H
    s = 4.0 / Y.mean()   # four counts per entry: no channel and no pixel without counts
    if simplex_W:
        H, H0 = H * s, H0 * s * H.mean() / H0.mean()
    else:
        W, W0 = W * s, W0 * s
    Y = Y * s
    X = Y * (0.5 + rng.random(Y.shape)) if opt.get("frac") else np.minimum(rng.poisson(Y), 255).astype(np.float64)
    assert (X.sum(axis=1) > 0).all() and (X.sum(axis=0) > 0).all()
    fixed_W = None
    if opt.get("fixed"):
        fixed_W = -np.ones((M, k))
        fixed_W[::7, 0] = 0.6 * W0.mean()
        fixed_W[3, :] = 1.3 * W0.mean()
    algo = {"pg": "projected_gradient", "bmd": "bmd"}.get(opt.get("algo"), "log_surrogate")
    kw = dict(simplex_H=not simplex_W, simplex_W=simplex_W, lambda_L=0.3, mu=0)
    Gd = G if m else np.eye(n)
    gamma = None
    if algo == "projected_gradient":   # step sizes as tests/test_gpu_fuzz.py draws them
        L = oc.laplacian_matrix(NX, NY)
        gh = np.abs(oc.gradH(X, Gd, W0, H0, mu=0, lambda_L=0.3, L=L)).max()
        gw = np.abs(oc.gradW(X, Gd, W0, H0)).max()
        gamma = [float(gh / 0.05), float(gw / (0.2 * W0.mean()))]
    return dict(X=X, G=G, Gd=Gd, W0=W0, H0=H0, rows=rows, fixed_W=fixed_W, algo=algo, kw=kw, gamma=gamma, k=k, n=n, m=m, M=M,
                no_scratch=bool(opt.get("no_scratch")))


def _engine(pr):
    from espm_amd.engine import MUEngine
    extra = {}
    if pr["algo"] == "projected_gradient":
        extra = dict(h_rule=2, sigmaL=pr["gamma"][0], pg_gamma_w=pr["gamma"][1])
    eng = MUEngine(pr["X"], pr["k"], G=pr["G"], shape_2d=(NX, NY), max_iter=6, tol=TOL, fixed_W=pr["fixed_W"], simplex_rows=pr["rows"],
                   bregman=pr["algo"] == "bmd", **extra, **pr["kw"])
    if pr["no_scratch"]:   # (as in test_local_w_update_equals_the_one_workgroup_finish)
        eng.st.w_scratch = None
    return eng


def _form_of(eng):
    name, d = eng.w_update_form()
    return name, ((d["threads"], d["rows"], d["channels"], d["gta_all_threads"]) if d else None)


def _oracle_step_w(pr):
    if pr["algo"] == "projected_gradient":
        return oc.proj_grad_step_w(pr["X"], pr["Gd"], pr["W0"], pr["H0"], pr["gamma"][1], simplex_W=False)
    return oc.multiplicative_step_w(pr["X"], pr["Gd"], pr["W0"], pr["H0"], simplex_W=pr["kw"]["simplex_W"], simplex_rows=pr["rows"],
                                    fixed_W=pr["fixed_W"], use_bregman=pr["algo"] == "bmd")


def _oracle_fit(pr, iters):
    model = _Rows(pr["Gd"], pr["rows"]) if pr["rows"] is not None else None
    extra = dict(gamma=pr["gamma"]) if pr["gamma"] else {}
    return oc.fit(pr["X"], pr["k"], G=None if model else pr["G"], W=pr["W0"].copy(), H=pr["H0"].copy(), shape_2d=(NX, NY), algo=pr["algo"],
                  exact_root=pr["algo"] == "log_surrogate", no_stop_criterion=True, max_iter=iters, tol=TOL, fixed_W=pr["fixed_W"],
                  physics_model=model, **extra, **pr["kw"])


def _worst(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|): at most 1 where assert_allclose passes."""
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref))))


def _check_products(eng, pr, Wn, tag):
    """gw_s and colsum_gw as the device left them against max(G W', gw_floor) / xscale in fp64 from the W' it returned."""
    n, k = pr["n"], pr["k"]
    Wn = Wn.astype(np.float64)
    gw = np.maximum(pr["G"].astype(np.float32).astype(np.float64) @ Wn if pr["m"] else Wn, 1e-30)   # (gw_floor; xscale = 1)
    rtol = ((pr["m"] or 1) + 2) * 2.0 ** -24
    got = eng.gw_s.cpu().numpy().astype(np.float64)
    cs = eng.colsum_gw.cpu().numpy()[:k]
    print(f"    {tag}: gw_s {_worst(got[:n, :k], gw, rtol, 1e-30):.3f} colsum_gw {_worst(cs, gw.sum(axis=0), rtol, 0.0):.3f} (of 1)")
    np.testing.assert_allclose(got[:n, :k], gw, rtol=rtol, atol=1e-30, err_msg=tag + ": rows of G W'")
    assert (got[n:, :k] > 0).all(), tag + ": padding rows of G W' must stay positive"
    np.testing.assert_allclose(cs, gw.sum(axis=0), rtol=rtol, err_msg=tag + ": colsum_gw")


def _run_case(case, expect=None):
    """Steps 1-3 of the module's docstring; returns the figures of the row's log line.  expect: the forms a knob moves the row to."""
    import torch
    t0 = time.perf_counter()
    pr = _problem(case)
    eng = _engine(pr)
    eng.load_state(pr["W0"], pr["H0"])
    # 1. the form
    form = _form_of(eng)
    SEEN[case["id"]] = (wc.build_of(case["k"]), ) + form
    assert eng.V.KP == wc.build_of(case["k"])
    if expect is None:
        assert form == (case["form"], case["detail"]), f"{case['id']}: the W update takes {form}"
    else:
        assert form[0] in expect, f"{case['id']}: the W update takes {form}, the knob should move it to {expect}"
    print(f"\nW-FORM {case['id']}: k={pr['k']} n={pr['n']} m={pr['m']} {case['opt']} store={eng.x_store} -> {form[0]} {form[1] or ''}")
    # 2. one W step
    Wn = eng.step_w_only()
    ref = _oracle_step_w(pr)
    step = _worst(Wn, ref, 3e-5, 1e-7)
    print(f"    one W step: {step:.3f} (of 1), max relative error {float(np.max(np.abs(Wn - ref) / ref)):.2e}")
    np.testing.assert_allclose(Wn, ref, rtol=3e-5, atol=1e-7, err_msg=case["id"] + ": one W step")
    if pr["fixed_W"] is not None:
        keep = pr["fixed_W"] >= 0
        assert np.array_equal(Wn[keep], pr["fixed_W"][keep].astype(np.float32))
    _check_products(eng, pr, Wn, "after step_w_only")
    # ... and one whole iteration: the form as the library's loop sequences it, its tail and its rel_W
    eng.load_state(pr["W0"], pr["H0"])
    eng.iterate(1, final_loss=False)
    torch.cuda.synchronize()
    W1 = eng.get_W()
    _check_products(eng, pr, W1, "after one iteration")
    W1d, W0f = W1.astype(np.float64), pr["W0"].astype(np.float32).astype(np.float64)
    rel_ref = np.max(np.abs(W1d - W0f) / (W1d + TOL * W1d.mean()))   # base.py:323
    rel_got = float(eng.history()["rel_W"][1])
    print(f"    rel_W of the first iteration: {rel_got:.9g} against {rel_ref:.9g} ({abs(rel_got - rel_ref) / rel_ref / 1e-6:.3f} of 1)")
    np.testing.assert_allclose(rel_got, rel_ref, rtol=1e-6, err_msg=case["id"] + ": rel_W")
    # 3. three iterations
    ref = _oracle_fit(pr, 3)
    if pr["algo"] == "projected_gradient":
        assert np.isfinite(ref["losses"]).all() and (np.diff(ref["losses"]) <= 0).all(), "redraw this row's seed: the oracle's losses must decrease"
    eng.iterate(2, final_loss=True)
    torch.cuda.synchronize()
    h = eng.history()
    We, He = eng.get_W().astype(np.float64), eng.get_H().astype(np.float64)
    wa = 2e-4 * np.abs(ref["W"]).mean()
    fig = dict(loss=_worst(h["loss"][1:], ref["losses"], LOSS_RTOL, 0.0), H=_worst(He, ref["H"], 2e-4, 2e-5), W=_worst(We, ref["W"], 2e-4, wa),
               rel_W=_worst(h["rel_W"][1:], ref["rel"][:, 0], 1e-3, 1e-5))
    dt = time.perf_counter() - t0
    print("    three iterations: " + " ".join(f"{key} {v:.3f}" for key, v in fig.items()) + f" (of 1)   {dt:.2f} s")
    np.testing.assert_allclose(h["loss"][1:], ref["losses"], rtol=LOSS_RTOL, err_msg=case["id"])
    np.testing.assert_allclose(He, ref["H"], rtol=2e-4, atol=2e-5, err_msg=case["id"])
    np.testing.assert_allclose(We, ref["W"], rtol=2e-4, atol=wa, err_msg=case["id"])
    np.testing.assert_allclose(h["rel_W"][1:], ref["rel"][:, 0], rtol=1e-3, atol=1e-5, err_msg=case["id"])
    assert h["bad"].sum() == 0
    return dict(form=form[0], step=step, seconds=dt, **fig)


@pytest.mark.parametrize("case", wc.CASES, ids=[c["id"] for c in wc.CASES])
def test_w_update_form(case):
    _run_case(case)


def test_every_form_is_reached():
    """The rows above, taken together, run every form and every instance of the register-resident finish that the plan can return in
    each of the three builds (w_form_cases.reachable: enumerated from the forms and the ROWS / CROWS / NT values built; the nt == 256
    instances exist only in the ESPM_WF_FEW_THREADS=256 A/B build).  Asked of the engines' own states, not of the table: a row that
    did not run in this process is asked for its form here."""
    for case in wc.CASES:
        if case["id"] not in SEEN:
            eng = _engine(_problem(case))
            SEEN[case["id"]] = (wc.build_of(case["k"]), ) + _form_of(eng)
    for kp in (8, 16, 32):
        got = {v[1:] for v in SEEN.values() if v[0] == kp}
        assert got == wc.reachable(kp), (kp, got ^ wc.reachable(kp))


def _knob_child(expect):
    """(child process, one of the knobs set) the three column-form rows, one line per row."""
    import traceback
    for case in wc.KNOB_CASES:
        try:
            out = dict(_run_case(case, expect=expect), status="passed", msg="")
        except Exception:
            out = dict(status="failed", msg=traceback.format_exc()[-1500:])
        print("CASE " + json.dumps(dict(out, id=case["id"])), flush=True)


@pytest.mark.parametrize("knob,expect", [("ESPM_W_GCOL", [wc.TWO]), ("ESPM_W_GSPLIT", [wc.REGS, wc.GENERAL])])
def test_escape_hatches_move_the_column_form(knob, expect):
    """README.md: ESPM_W_GCOL=0 keeps the two launches where the column form would run, ESPM_W_GSPLIT=0 the one workgroup where a
    many-workgroup form would.  The knobs are read once per process: one child per knob runs the three column-form rows, asserts that
    the form moved, and holds the form it moved to to the same three steps."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_w_update_forms as t; t._knob_child(%r)" % (
        here, os.path.dirname(here), expect)
    run = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{knob: "0"}), capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stderr[-3000:]
    cases = [json.loads(ln[5:]) for ln in run.stdout.splitlines() if ln.startswith("CASE ")]
    assert len(cases) == len(wc.KNOB_CASES) and all(c["status"] == "passed" for c in cases), "\n".join(c["id"] + ": " + c["msg"] for c in cases if c["status"] != "passed")
    assert {c["form"] for c in cases} <= set(expect)
