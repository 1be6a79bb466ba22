"""Do the estimator's post-fit methods compute the same thing in two trees?  The record behind moving them from estimators/base.py to
estimators/analysis.py (profiles/estimator_analysis_equal.log) and behind giving the analysis modules one upload
(profiles/image_host_equal.log).

    python tools/analysis/estimator_analysis_equal.py run OUT.npz [--root TREE]
    python tools/analysis/estimator_analysis_equal.py compare PARENT.npz PARENT_AGAIN.npz NEW.npz [--out profiles/estimator_analysis_equal.log]

``run`` imports espm_amd from TREE (default: this tree) and, under both values of ``hspy_comp`` and of ``normalize``, once with an identity G
and once with an 8-column dictionary (8 configurations), on a 32-channel, 16 x 16 pixel Poisson image with 3 components:

  fit/     SmoothNMF(max_iter=20).fit_transform, then on that estimator pixel_diagnostics, spectral_diagnostics and attribute_counts (each
           with the counts and with X=None), assign_counts, simulate, calibrate_deviance(n_rep=8), line_maps (a raw and a
           background-corrected window), region_spectra (three regions), residual_components(n_vectors=2), presence_maps with "em" and
           with "newton", and bootstrap(n_boot=3);
  binned/  fit_binned with bin (2, 2) on a fresh estimator;   split/  fit_split with q = 0.8 on a fresh estimator;
  hand/    the same methods, which do not refit the image, on an estimator whose G_, W_, H_, X_ and norm_factor_ are set by hand (fp32
           W_ and H_, and an fp32 G_ for the dictionary): functions of their inputs alone.

After every call every public attribute ending in "_" and every returned value is written to OUT.npz under configuration/stage/name.

``compare`` takes two runs of the parent and one of the new tree.  A key the parent reproduces bit for bit must be bit-equal in the new
tree; a key it does not must agree within the parent's own run-to-run difference, which is written down.  The keys under hand/ of the
methods that fit nothing (all but bootstrap) must be bit-equal whatever the parent does.  Exit status 1 on any miss."""
import argparse
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N, SHAPE, K, M = 32, (16, 16), 3, 8
P = SHAPE[0] * SHAPE[1]
LINES = [((5, 9), None), ((12, 16), ((8, 11), (18, 21)))]   # channel windows of line_maps: raw, and with two background windows
REGIONS = np.arange(P) % 3                                   # the label map of region_spectra


def problem(dictionary):
    """Counts (N, P) uint16, the dictionary (N, M) or None, and a model (W, H) near the truth to set by hand."""
    rng = np.random.default_rng(11)
    ell = np.linspace(0.0, 1.0, N)[:, None]
    G = None
    if dictionary:
        G = np.exp(-0.5 * ((ell - np.linspace(0.1, 0.9, M)[None, :]) / 0.08) ** 2) + 0.02
    W = rng.uniform(0.2, 1.0, (M if dictionary else N, K))
    W /= (W if G is None else G @ W).sum(axis=0, keepdims=True)
    H = rng.uniform(0.05, 1.0, (K, P))
    H /= H.sum(axis=0, keepdims=True)
    D = W if G is None else G @ W
    X = rng.poisson(60.0 * D @ H).astype(np.uint16)
    return X, G, 60.0 * W, H


def numeric(value):
    """value as a numeric array, or None."""
    if value is None or isinstance(value, (str, dict)):
        return None
    if hasattr(value, "detach"):
        value = value.detach().cpu().numpy()
    try:
        a = np.asarray(value)
    except Exception:
        return None
    return a if a.dtype.kind in "biuf" else None


class Record:
    def __init__(self):
        self.items = {}

    def put(self, key, value):
        if isinstance(value, dict):
            for name, v in value.items():
                self.put(f"{key}.{name}", v)
            return
        a = numeric(value)
        if a is not None:
            self.items[key] = a

    def state(self, prefix, est, returned=None):
        for name, value in vars(est).items():
            if name.endswith("_") and not name.startswith("_"):
                self.put(f"{prefix}/attr/{name}", value)
        if returned is not None:
            self.put(f"{prefix}/returned", returned)


def analyses(rec, prefix, est, Xc):
    """The methods that leave the image's fit alone; Xc: the counts, oriented as the estimator reads them."""
    for name in ("pixel_diagnostics", "spectral_diagnostics", "attribute_counts"):
        rec.state(f"{prefix}/{name}(X)", est, getattr(est, name)(Xc))
        rec.state(f"{prefix}/{name}(None)", est, getattr(est, name)())
    rec.state(f"{prefix}/assign_counts", est, est.assign_counts(Xc, seed=3))
    rec.state(f"{prefix}/simulate", est, est.simulate(seed=4, replicate=1))
    rec.state(f"{prefix}/calibrate_deviance", est, est.calibrate_deviance(Xc, n_rep=8, seed=5))
    rec.state(f"{prefix}/line_maps", est, est.line_maps(LINES, Xc))
    rec.state(f"{prefix}/region_spectra", est, est.region_spectra(REGIONS, Xc))
    rec.state(f"{prefix}/residual_components", est, est.residual_components(n_vectors=2, X=Xc))
    for method in ("em", "newton"):
        rec.state(f"{prefix}/presence_maps({method})", est, est.presence_maps(Xc, method=method))
    fitted = {n: np.array(getattr(est, n), copy=True) for n in ("G_", "W_", "H_", "X_")}
    rec.state(f"{prefix}/bootstrap", est, est.bootstrap(n_boot=3, seed=6, return_samples=True))
    assert all(np.array_equal(getattr(est, n), v) for n, v in fitted.items()), "bootstrap changed a fitted attribute"


def run(out):
    from espm_amd.estimators import SmoothNMF
    import espm_amd
    rec = Record()
    for hspy, norm, dictionary in itertools.product((False, True), (False, True), (False, True)):
        cfg = f"hspy_comp={int(hspy)},normalize={int(norm)},G={'dictionary' if dictionary else 'identity'}"
        X, G, Wm, Hm = problem(dictionary)
        Xc = np.ascontiguousarray(X.T) if hspy else X
        make = lambda: SmoothNMF(n_components=K, shape_2d=SHAPE, max_iter=20, G=G, normalize=norm, hspy_comp=hspy, verbose=0,  # noqa: E731
                                 random_state=0)
        est = make()
        rec.state(f"{cfg}/fit/fit_transform", est, est.fit_transform(Xc.astype(np.float32)))
        analyses(rec, f"{cfg}/fit", est, Xc)
        est = make()
        rec.state(f"{cfg}/binned/fit_binned", est, est.fit_binned(Xc.astype(np.float32), (2, 2)))
        est = make()
        rec.state(f"{cfg}/split/fit_split", est, est.fit_split(Xc, q=0.8, seed=7))
        est = make()
        est._identity_G, est.physics_model_ = G is None, None
        est.G_ = np.eye(N) if G is None else G.astype(np.float32)
        est.W_, est.H_ = Wm.astype(np.float32), Hm.astype(np.float32)
        est.norm_factor_ = 0.125
        est.X_ = X.astype(np.float32) * (est.norm_factor_ if norm else 1.0)
        analyses(rec, f"{cfg}/hand", est, Xc)
        print(cfg, "done", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **rec.items)
    print(f"{len(rec.items)} arrays from {os.path.dirname(os.path.abspath(espm_amd.__file__))} -> {out}")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def distance(a, b):
    """Largest |a - b| relative to the largest |a| (0 for equal bits; inf for another shape, dtype or NaN pattern)."""
    if same_bits(a, b):
        return 0.0
    if a.shape != b.shape or a.dtype != b.dtype:
        return np.inf
    a, b = a.astype(np.float64), b.astype(np.float64)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return np.inf
    with np.errstate(invalid="ignore"):
        diff = np.where(a == b, 0.0, np.abs(a - b))[~np.isnan(a)]   # (equal infinities are equal)
    scale = np.abs(a[np.isfinite(a)]).max(initial=0.0)
    return float(diff.max(initial=0.0) / (scale if scale > 0 else 1.0))


def compare(parent, again, new, out):
    runs = [dict(np.load(f)) for f in (parent, again, new)]
    lines, missed = [], 0
    if not (set(runs[0]) == set(runs[1]) == set(runs[2])):
        lines.append(f"MISS: the runs hold different keys: {sorted(set(runs[0]) ^ set(runs[2]))[:10]} ...")
        missed += 1
    keys = sorted(set(runs[0]) & set(runs[1]) & set(runs[2]))
    groups = {}
    for key in keys:
        cfg, stage, call = key.split("/")[:3]
        pure = stage == "hand" and not call.startswith("bootstrap")
        d_parent, d_new = distance(runs[0][key], runs[1][key]), distance(runs[0][key], runs[2][key])
        ok = d_new == 0.0 if (pure or d_parent == 0.0) else d_new <= d_parent
        if not ok:
            missed += 1
            lines.append(f"MISS {key}: parent vs parent {d_parent:.3e}, parent vs new {d_new:.3e}" + (" (must be bit-equal)" if pure else ""))
        g = groups.setdefault((stage, call), [0, 0, 0.0, 0.0])
        g[0] += 1
        g[1] += d_new == 0.0
        g[2], g[3] = max(g[2], d_parent), max(g[3], d_new)
    head = [f"estimator_analysis_equal: {parent} and {again} (parent, twice) against {new}",
            f"{len(keys)} arrays in 8 configurations (hspy_comp x normalize x identity / dictionary G); {N} channels, {SHAPE[0]} x {SHAPE[1]} pixels, k = {K}",
            "", f"{'stage':8s} {'call':30s} {'arrays':>7s} {'bit-equal':>10s} {'parent/parent':>14s} {'parent/new':>11s}"]
    for (stage, call), (n, eq, dp, dn) in sorted(groups.items()):
        head.append(f"{stage:8s} {call:30s} {n:7d} {eq:10d} {dp:14.3e} {dn:11.3e}")
    reproducible = all(g[2] == 0.0 for g in groups.values())
    head += ["", "the parent reproduces itself bit for bit in every array: bit equality demanded everywhere" if reproducible else
             "the parent does not reproduce itself everywhere: where parent/parent > 0 that difference (relative to the array's largest entry) is the bound",
             f"RESULT: {'equal' if not missed else f'{missed} MISSED'}"]
    text = "\n".join(head + lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)
    return 1 if missed else 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("out")
    r.add_argument("--root", default=HERE)
    c = sub.add_parser("compare")
    c.add_argument("files", nargs=3)
    c.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.cmd == "compare":
        sys.exit(compare(*args.files, args.out))
    sys.path.insert(0, os.path.abspath(args.root))
    run(args.out)


if __name__ == "__main__":
    main()
