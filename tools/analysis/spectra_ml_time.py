"""Time of espm_spectra_ml_pass (csrc/mu_spectra_ml.hip) against its yardstick espm_channel_diagnostics (csrc/mu_diag_chan.hip), and
of ``spectra_ml.presence`` end to end, at the headline image (2048 channels x 512^2 pixels; bench.py's dose of 500 counts per pixel).

    python tools/analysis/spectra_ml_time.py [--size n,nx,ny] [--k 5] [--m 12] [--runs 5] [--calls 10] [--out FILE]

1. The pass.  X is device-resident 8-bit synthetic Poisson counts; for each layout the two entry points (each the pass and the
   reduction of its pixel chunks) are timed INTERLEAVED in one process: a window of --calls calls of the one, then of the other, --runs
   times, HIP events around each window.  Reported: min - max over the windows per entry point, the ratio of the minima, and the
   yardstick's own run-to-run spread.  Arithmetic alone predicts (15 + k + 1) / 15: the new pass adds k FMAs and one multiply per
   entry.  The sums are compared with torch fp64 on a corner first, and the two layouts with each other bit for bit.
2. End to end.  A synthetic dictionary of --m Gaussian lines, X ~ Poisson(G W H): ``presence`` over all m k entries from W = 1 - total
   wall time, fits, passes, and the share spent inside the device pass (HIP events around every call of it) against the rest (the
   dense algebra in torch fp64 and the one read-back per pass)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from espm_amd import _lib, spectra_ml  # noqa: E402
from espm_amd.conf import log_shift  # noqa: E402
from espm_amd.engine import _ptr, _stream, require_gpu  # noqa: E402

from pixel_diagnostics_time import CODES, COUNTS, draw, model  # noqa: E402  (the same image as the diagnostics)
from spectral_diagnostics_time import kernel as yardstick  # noqa: E402


def new_pass(X, layout, D, H, out, un, scratch):
    n, p = (X.shape[0], X.shape[1]) if layout == "cm" else (X.shape[1], X.shape[0])
    _lib.check(_lib.lib.espm_spectra_ml_pass(_ptr(X), CODES[X.dtype], _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM, int(X.stride(0)),
                                             n, p, _ptr(D), _ptr(H), D.shape[1], float(log_shift), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                             _ptr(out[3]), _ptr(out[4]), _ptr(un), _ptr(scratch), scratch.numel() * 8, _stream()))


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def corner(X, D, H, nc, pc):
    x = X[:nc, :pc].to(torch.float64)
    y = (D[:nc] @ H[:, :pc]).clamp_min(log_shift)
    w = x / y
    return 2.0 * (torch.xlogy(x, w) - x + y).sum(dim=1), w @ H[:, :pc].T, torch.einsum("ip,jp,cp->cij", H[:, :pc], H[:, :pc], w / y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,512,512")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--m", type=int, default=12)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    require_gpu()
    n, nx, ny = (int(v) for v in args.size.split(","))
    p, k, m = nx * ny, args.k, args.m
    nt = k * (k + 1) // 2
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"spectra ML pass, {n} channels x {nx} x {ny} pixels, k = {k}, 8-bit X, 500 counts per pixel, {args.runs} interleaved windows of "
        f"{args.calls} calls, {torch.cuda.get_device_name(0)}")
    g = torch.Generator(device="cuda").manual_seed(k)
    D, H = model(n, p, k, g)
    X8 = draw(D, H, g)
    rel = lambda a, b: float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())   # noqa: E731
    nc, pc = min(64, n), min(16384, p)
    oc = tuple(torch.empty(s, dtype=torch.float64, device="cuda") for s in (nc, nc, nc, (nc, k), (nc, nt)))
    un = torch.zeros(1, dtype=torch.int64, device="cuda")
    sc = torch.empty(_lib.lib.espm_spectra_ml_pass_scratch(nc, pc, k) // 8, dtype=torch.float64, device="cuda")
    new_pass(X8[:nc, :pc].contiguous(), "cm", D[:nc].contiguous(), H[:, :pc].contiguous(), oc, un, sc)
    dev, Q, A = corner(X8, D, H, nc, pc)
    il, jl = torch.tril_indices(k, k)
    say(f"  corner ({nc} x {pc}) against torch fp64: max rel. difference deviance {rel(oc[0], dev):.1e}, Q {rel(oc[3], Q):.1e}, "
        f"A {rel(oc[4], A[:, il, jl]):.1e}; unmodelled {int(un.item())}")
    del oc, sc, dev, Q, A
    out = tuple(torch.empty(s, dtype=torch.float64, device="cuda") for s in (n, n, n, (n, k), (n, nt)))
    yout = tuple(torch.empty(s, dtype=torch.float64, device="cuda") for s in (n, n, n, (n, nt)))
    scratch = torch.empty(_lib.lib.espm_spectra_ml_pass_scratch(n, p, k) // 8, dtype=torch.float64, device="cuda")
    yscratch = torch.empty(_lib.lib.espm_channel_diagnostics_scratch(n, p, k) // 8, dtype=torch.float64, device="cuda")
    first = None
    for layout in ("cm", "pm"):
        X = X8 if layout == "cm" else X8.t().contiguous()
        a = lambda: new_pass(X, layout, D, H, out, un, scratch)   # noqa: E731
        b = lambda: yardstick(X, layout, D, H, yout, yscratch)   # noqa: E731
        for _ in range(3):
            a(), b()
        torch.cuda.synchronize()
        got = torch.cat([o.reshape(-1) for o in out]).clone()
        same = "" if first is None else f"; bit-equal to cm: {bool(torch.equal(got, first))}"
        first = got if first is None else first
        ta, tb = [], []
        for _ in range(args.runs):
            ta.append(window(a, args.calls))
            tb.append(window(b, args.calls))
        say(f"  {layout}: espm_spectra_ml_pass {min(ta):.3f} - {max(ta):.3f} ms, espm_channel_diagnostics {min(tb):.3f} - {max(tb):.3f} ms "
            f"(spread {100 * (max(tb) / min(tb) - 1):.1f} %); ratio {min(ta) / min(tb):.3f} against (15 + k + 1) / 15 = {(16 + k) / 15:.3f}; "
            f"scratch {scratch.numel() * 8 / 1e6:.0f} MB{same}")
        del X
    del out, yout, scratch, yscratch, X8, first, got
    torch.cuda.empty_cache()

    # ---- end to end: presence() with a synthetic dictionary -------------------------------------------------------------------------
    c = torch.arange(n, device="cuda", dtype=torch.float64)[:, None]
    G = torch.exp(-0.5 * ((c - (torch.arange(m, device="cuda", dtype=torch.float64)[None, :] + 0.5) * n / m) / (n / (6.0 * m))) ** 2) + 0.05
    W = torch.rand((m, k), generator=g, device="cuda", dtype=torch.float64) ** 2 + 0.05
    W[1, 2 % k] = W[m - 2, 0] = 0.0   # two entries planted at zero
    W = W * (COUNTS / (G @ W).sum(dim=0, keepdim=True))
    X = draw((G @ W).contiguous(), H, g)
    spent = []
    inner = spectra_ml._Solver.device_pass

    def timed_pass(self, Wd):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = inner(self, Wd)
        e1.record()
        spent.append((e0, e1))
        return r

    spectra_ml._Solver.device_pass = timed_pass
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = spectra_ml.presence(X, G.cpu().numpy(), H.cpu().numpy())
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        spectra_ml._Solver.device_pass = inner
    in_pass = sum(a.elapsed_time(b) for a, b in spent) * 1e-3
    lr = res["lr"]
    say(f"presence(), dictionary of m = {m}: {len(res['entries'])} tested entries, {len(res['n_pass'])} fits, {int(res['n_pass'].sum())} passes "
        f"(full fit {int(res['n_pass'][0])}, nested at most {int(res['n_pass'][1:].max())}), all converged: {bool(res['converged'].all())}")
    say(f"  total {total:.2f} s (the upload of the resident image and the count of N included); in the device pass (with G W and the "
        f"unpacking of A) {in_pass:.2f} s = {100 * in_pass / total:.0f} %, the rest (dense algebra in torch fp64, one read-back per "
        f"pass, upload) {total - in_pass:.2f} s = {100 * (1 - in_pass / total):.0f} %; {1e3 * in_pass / len(spent):.2f} ms per pass")
    say(f"  lr of the two planted-absent entries: {lr[1, 2 % k]:.3g}, {lr[m - 2, 0]:.3g}; smallest lr of the others: "
        f"{float(min(v for (e, j), v in zip(res['entries'], lr[res['entries'][:, 0], res['entries'][:, 1]]) if (e, j) not in ((1, 2 % k), (m - 2, 0)))):.3g}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
