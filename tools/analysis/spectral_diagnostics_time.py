"""Time of espm_channel_diagnostics (csrc/mu_diag_chan.hip) at the headline image (2048 channels x 512^2 pixels; bench.py's dose of 500
counts per pixel) for k = 5 and 8, 8-bit and fp32 X, in both layouts.

    python tools/analysis/spectral_diagnostics_time.py [--size n,nx,ny] [--runs 5] [--calls 20] [--out FILE]

X is device-resident (synthetic Poisson counts drawn on the device); every configuration is warmed up, then timed --runs times with
HIP events around --calls back-to-back calls (each the pass and the reduction of its pixel chunks), so that a window holds tens of
milliseconds of work; the time per call, min - max over the windows, is reported, with
  * X's bytes / time as a share of the 8 TB/s HBM peak (the image is read once; the scratch of partial sums is written and read once
    more and is listed on its own),
  * the fp64 work / time as a share of the 78.6 TFLOP/s vector fp64 peak, counting per entry k + k (k + 1) / 2 + 6 FMAs (2 flop
    each) - the division and the logarithm (where x > 0) are on top and not counted.
The kernel's sums are compared with torch on a corner of the image (fp64, 64 channels x 16384 pixels) before anything is timed, and
the two layouts with each other bit for bit."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from espm_amd import _lib  # noqa: E402
from espm_amd.conf import log_shift  # noqa: E402
from espm_amd.engine import _ptr, _stream, require_gpu  # noqa: E402

from pixel_diagnostics_time import CODES, draw, model  # noqa: E402  (the same image as the pixel side)

HBM_PEAK, FP64_PEAK = 8e12, 78.6e12


def timed(fn, runs, calls):
    """(min, max) over ``runs`` windows of the time per call in ms, ``calls`` calls per pair of events."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return min(ms), max(ms)


def kernel(X, layout, D, H, out, scratch):
    n, p = (X.shape[0], X.shape[1]) if layout == "cm" else (X.shape[1], X.shape[0])
    _lib.check(_lib.lib.espm_channel_diagnostics(_ptr(X), CODES[X.dtype], _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM,
                                                 int(X.stride(0)), n, p, _ptr(D), _ptr(H), D.shape[1], float(log_shift), _ptr(out[0]),
                                                 _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _ptr(scratch), scratch.numel() * 8, _stream()))


def corner(X, D, H, nc=64, pc=16384):
    """dev, sum x, sum y and M of the first ``nc`` channels over the first ``pc`` pixels with torch in fp64 (X channel-major)."""
    x = X[:nc, :pc].to(torch.float64)
    y = (D[:nc] @ H[:, :pc]).clamp_min(log_shift)
    dev = 2.0 * (torch.xlogy(x, x / y) - x + y).sum(dim=1)
    M = torch.einsum("ip,jp,cp->cij", H[:, :pc], H[:, :pc], 1.0 / y)
    return dev, x.sum(dim=1), y.sum(dim=1), M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,512,512")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    require_gpu()
    n, nx, ny = (int(v) for v in args.size.split(","))
    p = nx * ny
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"channel diagnostics, {n} channels x {nx} x {ny} pixels, 500 counts per pixel, pixel chunks of {_lib.CDIAG_PCHUNK}, "
        f"{args.runs} windows of {args.calls} calls, {torch.cuda.get_device_name(0)}")
    for k in (5, 8):
        g = torch.Generator(device="cuda").manual_seed(k)
        D, H = model(n, p, k, g)
        X8 = draw(D, H, g)
        nt = k * (k + 1) // 2
        say(f"k = {k}: {float((X8 != 0).float().mean()):.3f} of the entries are non-zero")
        # the kernel on the corner against torch
        nc, pc = min(64, n), min(16384, p)
        Xc = X8[:nc, :pc].contiguous()
        oc = tuple(torch.empty(s, dtype=torch.float64, device="cuda") for s in (nc, nc, nc, (nc, nt)))
        sc = torch.empty(_lib.lib.espm_channel_diagnostics_scratch(nc, pc, k) // 8, dtype=torch.float64, device="cuda")
        kernel(Xc, "cm", D[:nc].contiguous(), H[:, :pc].contiguous(), oc, sc)
        dev, xs, ys, M = corner(X8, D, H, nc, pc)
        il, jl = torch.tril_indices(k, k)
        rel = lambda a, b: float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())   # noqa: E731
        say(f"  corner ({nc} x {pc}) against torch fp64: max rel. difference deviance {rel(oc[0], dev):.1e}, sum x {rel(oc[1], xs):.1e}, "
            f"sum y {rel(oc[2], ys):.1e}, M {rel(oc[3], M[:, il, jl]):.1e}")
        del Xc, oc, sc, dev, xs, ys, M
        out = tuple(torch.empty(s, dtype=torch.float64, device="cuda") for s in (n, n, n, (n, nt)))
        sbytes = int(_lib.lib.espm_channel_diagnostics_scratch(n, p, k))
        scratch = torch.empty(sbytes // 8, dtype=torch.float64, device="cuda")
        flop = 2.0 * (k + nt + 6) * n * p
        for dtype in (torch.uint8, torch.float32):
            Xd = X8 if dtype == torch.uint8 else X8.to(dtype)
            first = None
            for layout in ("cm", "pm"):
                X = Xd if layout == "cm" else Xd.t().contiguous()
                kernel(X, layout, D, H, out, scratch)
                torch.cuda.synchronize()
                got = torch.cat([o.reshape(-1) for o in out]).clone()
                same = "" if first is None else f", bit-equal to cm: {bool(torch.equal(got, first))}"
                first = got if first is None else first
                lo, hi = timed(lambda: kernel(X, layout, D, H, out, scratch), args.runs, args.calls)
                xb = X.numel() * X.element_size()
                say(f"  k={k} {str(dtype).split('.')[-1]:8s} {layout}: {lo:8.3f} - {hi:8.3f} ms; X {xb / 1e9:.3f} GB -> {xb / lo / 1e6:.0f} GB/s = "
                    f"{100 * xb / (lo * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s (scratch {sbytes / 1e6:.0f} MB on top); "
                    f"{flop / lo / 1e9:.1f} TFLOP/s fp64 = {100 * flop / (lo * 1e-3) / FP64_PEAK:.1f} % of 78.6{same}")
                del X
            del Xd, first
        del X8, D, H, out, scratch
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
