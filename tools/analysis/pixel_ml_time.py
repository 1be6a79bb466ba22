"""Time of espm_pixel_ml (csrc/mu_pixel_ml.hip) and espm_pixel_ml_newton (csrc/mu_pixel_ml_newton.hip) at the headline image (2048
channels x 512^2 pixels, k = 5, 8-bit X): the time of one pass over the image, the passes the pixels need at tol = 1e-3, and the whole
of ``presence.presence`` (k + 1 nested fits) - against ONE espm_pixel_diagnostics pass over the same image in the same process, the
yardstick: an EM pass does strictly less arithmetic per entry (2 k FMAs, one division, one logarithm against that plus
k (k + 1) / 2 FMAs), a Newton pass the two together.

    python tools/analysis/pixel_ml_time.py [--size n,nx,ny] [--k 5] [--counts 500] [--runs 3] [--max-pass 20000] [--method em|newton|both]
                                           [--no-presence] [--pinned] [--simplex] [--out FILE]

``--pinned``: also espm_pixel_ml_pinned (csrc/mu_pixel_ml_pinned.hip) - the time of one pinned pass against one Newton pass, the two
INTERLEAVED in one process (Newton with 1 pass, pinned with 1, Newton with 3, pinned with 3, and again: the same walk plus one
output, so the two should agree), the last component held at 1.5 times its start; and ``presence.intervals`` end to end with its
evaluation and pass counts per percentile of the pixels.

``--simplex``: also espm_pixel_ml_simplex (csrc/mu_pixel_ml_simplex.hip) on the same image with the spectra brought to the data's
dose (D times mean N / mean s: the simplex model has no scale per pixel) - the time of one simplex pass, with the last component
pinned at 0.3 and with nothing pinned, against one pinned pass, the three INTERLEAVED in one process as above (the same walk; the
additions are between the walks); then ``presence.presence(method="simplex")`` and ``presence.intervals(simplex=True)`` end to end.

X is device-resident (synthetic Poisson counts drawn on the device from ``pixel_diagnostics_time.model``).  The time per pass is the
difference of two calls from the same fresh state, with 4 and with 12 passes (EM) or with 1 and with 3 (Newton, whose pixels stop
within a handful), over the passes between them (the count of pixels not done is printed with both: a pixel that stopped in between
takes no further pass) - the first call's walk for N and the launch are in both and cancel.  Every number
is min - max over --runs after a warm-up, HIP events around the calls."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pixel_diagnostics_time as pdt  # noqa: E402
from espm_amd import _lib, presence  # noqa: E402
from espm_amd.conf import log_shift  # noqa: E402
from espm_amd.engine import _ptr, _stream, require_gpu  # noqa: E402


def passes_call(X, D, s, H, state, n_pass, tol, method="em"):
    dv, gp, passes, done, counters = state
    n, p = X.shape
    args = (_ptr(X), pdt.CODES[X.dtype], _lib.LAYOUT_CM, int(X.stride(0)), n, p, _ptr(D), s.ctypes.data, D.shape[1], (1 << D.shape[1]) - 1,
            float(log_shift), tol, n_pass, _ptr(H), _ptr(dv), _ptr(gp), _ptr(passes), _ptr(done), _ptr(counters))
    if method == "newton":
        extra = torch.empty((D.shape[1] + _lib.PMLN_STATE_EXTRA, p), dtype=torch.float64, device="cuda")
        _lib.check(_lib.lib.espm_pixel_ml_newton(*args, _ptr(extra), extra.numel() * 8, _stream()))
    else:
        _lib.check(_lib.lib.espm_pixel_ml(*args, _stream()))


def pinned_call(X, D, s, H, state, t, slope, n_pass, tol):
    dv, gp, passes, done, counters = state
    n, p = X.shape
    k = D.shape[1]
    extra = torch.empty((k + _lib.PMLN_STATE_EXTRA, p), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib.espm_pixel_ml_pinned(_ptr(X), pdt.CODES[X.dtype], _lib.LAYOUT_CM, int(X.stride(0)), n, p, _ptr(D), s.ctypes.data, k,
                                             (1 << (k - 1)) - 1, k - 1, _ptr(t), float(log_shift), tol, n_pass, _ptr(H), _ptr(dv), _ptr(gp),
                                             _ptr(slope), _ptr(passes), _ptr(done), _ptr(counters), _ptr(extra), extra.numel() * 8, _stream()))


def simplex_call(X, D, s, H, state, t, slope, n_pass, tol):
    """espm_pixel_ml_simplex with the last component pinned at ``t``, or with nothing pinned (``t`` None)."""
    dv, gp, passes, done, counters = state
    n, p = X.shape
    k = D.shape[1]
    extra = torch.empty((k + _lib.PMLN_STATE_EXTRA, p), dtype=torch.float64, device="cuda")
    mask, pin = ((1 << k) - 1, -1) if t is None else ((1 << (k - 1)) - 1, k - 1)
    _lib.check(_lib.lib.espm_pixel_ml_simplex(_ptr(X), pdt.CODES[X.dtype], _lib.LAYOUT_CM, int(X.stride(0)), n, p, _ptr(D), s.ctypes.data, k,
                                              mask, pin, None if t is None else _ptr(t), float(log_shift), tol, n_pass, _ptr(H), _ptr(dv),
                                              _ptr(gp), None if t is None else _ptr(slope), _ptr(passes), _ptr(done), _ptr(counters),
                                              _ptr(extra), extra.numel() * 8, _stream()))


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def fresh(p, k, H0):
    return H0.clone(), (torch.zeros(p, dtype=torch.float64, device="cuda"), torch.zeros(p, dtype=torch.float64, device="cuda"),
                        torch.zeros(p, dtype=torch.int32, device="cuda"), torch.zeros(p, dtype=torch.uint8, device="cuda"),
                        torch.zeros(3, dtype=torch.int64, device="cuda"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,512,512")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--counts", type=float, default=500.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--max-pass", type=int, default=presence.MAX_PASS)
    ap.add_argument("--method", choices=("em", "newton", "both"), default="em")
    ap.add_argument("--no-presence", action="store_true")
    ap.add_argument("--pinned", action="store_true")
    ap.add_argument("--simplex", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    require_gpu()
    n, nx, ny = (int(v) for v in args.size.split(","))
    p, k, tol = nx * ny, args.k, 1e-3

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").close()

    def say(text):
        print(text, flush=True)
        if args.out:   # (line by line: the nested fits take a while)
            with open(args.out, "a") as f:
                f.write(text + "\n")

    pdt.COUNTS = args.counts
    g = torch.Generator(device="cuda").manual_seed(k)
    D, Ht = pdt.model(n, p, k, g)
    X = pdt.draw(D, Ht, g)
    say(f"pixel ML, {n} channels x {nx} x {ny} pixels, k = {k}, {args.counts:.0f} counts per pixel, uint8 channel-major, tol = {tol:g}, "
        f"{torch.cuda.get_device_name(0)}")
    # the yardstick: one pixel diagnostics pass
    out = (torch.empty(p, dtype=torch.float64, device="cuda"), torch.empty((k, p), dtype=torch.float64, device="cuda"),
           torch.zeros(1, dtype=torch.int32, device="cuda"))
    lo, hi = pdt.timed(lambda: pdt.kernel(X, "cm", D, Ht, False, out), args.runs)
    say(f"  espm_pixel_diagnostics, one pass: {lo:8.3f} - {hi:8.3f} ms")
    diag = (lo, hi)
    s = np.ascontiguousarray(D.sum(dim=0).cpu().numpy())
    H0 = (X.sum(dim=0, dtype=torch.float64) / float(s.sum()))[None, :].repeat(k, 1).contiguous()
    for method in (("em", "newton") if args.method == "both" else (args.method,)):
        entry = "espm_pixel_ml" if method == "em" else "espm_pixel_ml_newton"
        # one pass
        t, (few, many) = {}, ((4, 12) if method == "em" else (1, 3))
        for n_pass in (few, many):
            def run():
                H, state = fresh(p, k, H0)
                passes_call(X, D, s, H, state, n_pass, tol, method)
                run.left = state[4]
            # (the allocation and the clone of the fresh state are inside the events of both calls and cancel in the difference)
            t[n_pass] = pdt.timed(run, args.runs)
            left = int(run.left[_lib.PML_NOT_DONE])
            say(f"  {entry}, {n_pass:2d} passes from a fresh state: {t[n_pass][0]:8.3f} - {t[n_pass][1]:8.3f} ms, {left} of {p} pixels not done")
        per = ((t[many][0] - t[few][0]) / (many - few), (t[many][1] - t[few][1]) / (many - few))
        say(f"  {method}: time per pass: {min(per):8.3f} - {max(per):8.3f} ms = {min(per) / diag[0]:.2f} of a pixel diagnostics pass")
        if not args.no_presence:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = presence.presence(X, D.cpu().numpy(), tol=tol, max_pass=args.max_pass, method=method)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            npass = res["n_pass"]
            q = np.percentile(npass[0], [50, 99, 100])
            say(f"  {method}: full fit: passes to the 50th / 99th / last percentile of the pixels: {q[0]:.0f} / {q[1]:.0f} / {q[2]:.0f}; "
                f"{res['converged'][0].mean():.6f} converged (max_pass {args.max_pass})")
            for j in range(k):
                qj = np.percentile(npass[1 + j], [50, 99, 100])
                say(f"  {method}: without component {j}: {qj[0]:.0f} / {qj[1]:.0f} / {qj[2]:.0f} passes; {res['converged'][1 + j].mean():.6f} converged")
            say(f"  {method}: presence, {k + 1} nested fits, read-backs included: {total:.2f} s; median lr per component {np.median(res['lr'], axis=1)}")
    if args.pinned and k >= 2:
        t = (1.5 * H0[k - 1]).contiguous()
        slope = torch.zeros(p, dtype=torch.float64, device="cuda")
        left = {}

        def newton(n_pass):
            H, state = fresh(p, k, H0)
            passes_call(X, D, s, H, state, n_pass, tol, "newton")
            left["newton", n_pass] = state[4]

        def pinned(n_pass):
            H, state = fresh(p, k, H0)
            pinned_call(X, D, s, H, state, t, slope, n_pass, tol)
            left["pinned", n_pass] = state[4]

        order = [("newton", newton, 1), ("pinned", pinned, 1), ("newton", newton, 3), ("pinned", pinned, 3)]
        for _, fn, n_pass in order:   # warm-up
            fn(n_pass)
        torch.cuda.synchronize()
        ms = {(name, n_pass): [] for name, _, n_pass in order}
        for _ in range(args.runs):
            for name, fn, n_pass in order:
                ms[name, n_pass].append(event_ms(lambda: fn(n_pass)))
        per = {}
        for name in ("newton", "pinned"):
            for n_pass in (1, 3):
                v = ms[name, n_pass]
                say(f"  interleaved, {name}, {n_pass} passes from a fresh state: {min(v):8.3f} - {max(v):8.3f} ms, "
                    f"{int(left[name, n_pass][_lib.PML_NOT_DONE])} of {p} pixels not done")
            d = [(b - a) / 2 for a, b in zip(ms[name, 1], ms[name, 3])]
            per[name] = (min(d), max(d))
            say(f"  interleaved, {name}: time per pass: {min(d):8.3f} - {max(d):8.3f} ms")
        say(f"  pinned / newton, time per pass: {per['pinned'][0] / per['newton'][0]:.3f} (min over min)")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = presence.intervals(X, D.cpu().numpy(), tol=tol, max_pass=args.max_pass)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        ne, npx = res["n_eval"].sum(axis=(0, 1)), res["n_pass"].sum(axis=(0, 1))
        qe, qp = np.percentile(ne, [50, 99, 100]), np.percentile(npx, [50, 99, 100])
        say(f"  intervals, level 0.95, {2 * k} ends per pixel, read-backs included: {total:.2f} s; {res['converged'].mean():.6f} of the ends converged")
        say(f"  intervals: pinned fits per pixel over all ends, 50th / 99th / last percentile: {qe[0]:.0f} / {qe[1]:.0f} / {qe[2]:.0f}; "
            f"passes: {qp[0]:.0f} / {qp[1]:.0f} / {qp[2]:.0f}; per end at most {res['n_eval'].max()} fits and {res['n_pass'].max()} passes")
        say(f"  intervals: lower end at 0 in {np.mean(res['lower'] == 0):.4f} of the entries; median width per component "
            f"{np.nanmedian(res['upper'] - res['lower'], axis=1)}")
    if args.simplex and k >= 2:
        Ds = (D * float(X.sum(dim=0, dtype=torch.float64).mean() / s.mean())).contiguous()
        ss = np.ascontiguousarray(Ds.sum(dim=0).cpu().numpy())
        Hs = torch.full((k, p), 1.0 / k, dtype=torch.float64, device="cuda")
        tp, ts = (1.5 * H0[k - 1]).contiguous(), torch.full((p,), 0.3, dtype=torch.float64, device="cuda")
        slope = torch.zeros(p, dtype=torch.float64, device="cuda")
        left = {}

        def make(name, n_pass):
            def fn():
                H, state = fresh(p, k, H0 if name == "pinned" else Hs)
                if name == "pinned":
                    pinned_call(X, D, s, H, state, tp, slope, n_pass, tol)
                else:
                    simplex_call(X, Ds, ss, H, state, ts if name == "simplex, pinned" else None, slope, n_pass, tol)
                left[name, n_pass] = state[4]
            return fn

        names = ("pinned", "simplex, pinned", "simplex")
        order = [(name, make(name, n_pass), n_pass) for n_pass in (1, 3) for name in names]
        for _, fn, _ in order:   # warm-up
            fn()
        torch.cuda.synchronize()
        ms = {(name, n_pass): [] for name, _, n_pass in order}
        for _ in range(args.runs):
            for name, fn, n_pass in order:
                ms[name, n_pass].append(event_ms(fn))
        per = {}
        for name in names:
            for n_pass in (1, 3):
                v = ms[name, n_pass]
                say(f"  interleaved, {name}, {n_pass} passes from a fresh state: {min(v):8.3f} - {max(v):8.3f} ms, "
                    f"{int(left[name, n_pass][_lib.PML_NOT_DONE])} of {p} pixels not done")
            d = [(b - a) / 2 for a, b in zip(ms[name, 1], ms[name, 3])]
            per[name] = (min(d), max(d))
            say(f"  interleaved, {name}: time per pass: {min(d):8.3f} - {max(d):8.3f} ms")
        for name in names[1:]:
            say(f"  {name} / pinned, time per pass: {per[name][0] / per['pinned'][0]:.3f} (min over min)")
        Dh = Ds.cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = presence.presence(X, Dh, tol=tol, max_pass=args.max_pass, method="simplex")
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        q = np.percentile(res["n_pass"][0], [50, 99, 100])
        qr = np.percentile(res["n_pass"][1:], [50, 99, 100])
        say(f"  simplex: presence, {k + 1} nested fits, read-backs included: {total:.2f} s; passes of the full fit, 50th / 99th / last percentile "
            f"of the pixels: {q[0]:.0f} / {q[1]:.0f} / {q[2]:.0f}; of a reduced fit: {qr[0]:.0f} / {qr[1]:.0f} / {qr[2]:.0f}; "
            f"{res['converged'].mean():.6f} converged; median lr per component {np.median(res['lr'], axis=1)}")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = presence.intervals(X, Dh, tol=tol, max_pass=args.max_pass, simplex=True)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        ne, npx = res["n_eval"].sum(axis=(0, 1)), res["n_pass"].sum(axis=(0, 1))
        qe, qp = np.percentile(ne, [50, 99, 100]), np.percentile(npx, [50, 99, 100])
        say(f"  simplex: intervals, level 0.95, {2 * k} ends per pixel, read-backs included: {total:.2f} s; {res['converged'].mean():.6f} of the ends "
            f"converged")
        say(f"  simplex: intervals: pinned fits per pixel over all ends, 50th / 99th / last percentile: {qe[0]:.0f} / {qe[1]:.0f} / {qe[2]:.0f}; "
            f"passes: {qp[0]:.0f} / {qp[1]:.0f} / {qp[2]:.0f}; per end at most {res['n_eval'].max()} fits and {res['n_pass'].max()} passes")
        say(f"  simplex: intervals: lower end at 0 in {np.mean(res['lower'] == 0):.4f} of the entries, upper end at 1 in "
            f"{np.mean(res['upper'] == 1):.4f}; median width per component {np.nanmedian(res['upper'] - res['lower'], axis=1)}")


if __name__ == "__main__":
    main()
