"""Time of the pixel-binning kernels (csrc/mu_binning.hip) at the headline image (2048 channels x 512^2 pixels; bench.py's dose of 500
counts per pixel), 8-bit and fp32 X, both layouts: espm_rebin_pixels at bin (4, 4), and espm_binning_sums over the default candidates
of espm_amd.binning (the square bins 1 .. 256: 256 passes and the totals' pass).

    python tools/analysis/binning_time.py [--size n,ny,nx] [--calls 20] [--out profiles/binning_time.log]

X is device-resident (synthetic Poisson counts drawn on the device).  Every configuration is warmed up, then every one of --calls
calls is timed between its own pair of HIP events; the median is reported (with the minimum and the maximum), as a share of the 8 TB/s
HBM peak on the call's ALGORITHMIC bytes: for the rebin X once and the binned image once; for the scan X once - what an algorithm
that formed every candidate's sums in one pass would read - and, next to it, the bytes the scan does read (X once per candidate and
once for the totals).  Single candidates are timed on their own to show where the scan's time goes.  Before anything is timed the
binned image is compared with torch on the whole image and the sums of four candidates with torch in fp64."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from espm_amd import _lib, binning  # noqa: E402
from espm_amd.engine import _ptr, _stream, require_gpu  # noqa: E402

from pixel_diagnostics_time import CODES, draw, model  # noqa: E402  (the same image as the diagnostics' timings)

HBM_PEAK = 8e12


def timed(fn, calls):
    """(median, min, max) in ms over ``calls`` calls, each between its own pair of events."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def _layout(layout):
    return _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM


def rebin_call(X, layout, n, ny, nx, bin, out):
    _lib.check(_lib.lib.espm_rebin_pixels(_ptr(X), CODES[X.dtype], _layout(layout), int(X.stride(0)), n, ny, nx, bin[0], bin[1], _ptr(out),
                                          _lib.DIAG_X_F32, int(out.stride(0)), _stream()))


def sums_call(X, layout, n, ny, nx, bins, out, scratch):
    _lib.check(_lib.lib.espm_binning_sums(_ptr(X), CODES[X.dtype], _layout(layout), int(X.stride(0)), n, ny, nx, bins.ctypes.data, len(bins),
                                          _ptr(out), _ptr(scratch), scratch.numel() * 8, _stream()))


def torch_sums(X8, n, ny, nx, b):
    """T1, T2, A, C of the channel-major 8-bit image for a square bin b that divides it, with torch in fp64."""
    x = X8.to(torch.float64)
    S = x.reshape(n, ny // b, b, nx // b, b).sum(dim=(2, 4))
    return float(x.sum()), float((x * x).sum()), float((S * S).sum() / (b * b)), float(S.sum() / (b * b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,512,512")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binning_time.log"))
    args = ap.parse_args()
    require_gpu()
    n, ny, nx = (int(v) for v in args.size.split(","))
    p = ny * nx
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"pixel binning, {n} channels x {ny} x {nx} pixels, 500 counts per pixel, {_lib.BIN_PARTS} workgroups per pass of the scan, "
        f"median (min - max) of {args.calls} calls, {torch.cuda.get_device_name(0)}")
    g = torch.Generator(device="cuda").manual_seed(5)
    D, H = model(n, p, 5, g)
    X8 = draw(D, H, g)
    del D, H
    say(f"{float(X8.to(torch.float32).mean()):.3f} counts per entry")
    bins = np.ascontiguousarray(np.asarray(binning.default_bins((ny, nx)), dtype=np.int32))
    nb = len(bins)
    gny, gnx = binning.binned_shape((ny, nx), (4, 4))
    # correctness first: the binned image and four candidates against torch
    out = torch.empty((n, gny * gnx), dtype=torch.float32, device="cuda")
    rebin_call(X8, "cm", n, ny, nx, (4, 4), out)
    ref = X8.reshape(n, gny, 4, gnx, 4).to(torch.float32).sum(dim=(2, 4)).reshape(n, -1) if ny % 4 == 0 and nx % 4 == 0 else None
    if ref is not None:
        say(f"rebin (4, 4) against torch: equal {bool(torch.equal(out, ref))}")
    del ref
    some = np.ascontiguousarray(np.asarray([(b, b) for b in (1, 4, 32, 256) if ny % b == 0 and nx % b == 0], dtype=np.int32))
    so = torch.empty(2 + 2 * len(some), dtype=torch.float64, device="cuda")
    sc = torch.empty(_lib.lib.espm_binning_sums_scratch(n, ny, nx, len(some)) // 8, dtype=torch.float64, device="cuda")
    sums_call(X8, "cm", n, ny, nx, some, so, sc)
    got = so.cpu().numpy()
    worst = 0.0
    for i, (b, _) in enumerate(some):
        t1, t2, a, c = torch_sums(X8, n, ny, nx, int(b))
        worst = max(worst, abs(got[0] - t1) / t1, abs(got[1] - t2) / t2, abs(got[2 + 2 * i] - a) / a, abs(got[3 + 2 * i] - c) / c)
    say(f"sums of the candidates {[int(b) for b, _ in some]} against torch fp64: max rel. difference {worst:.1e}")
    del so, sc, out
    res = torch.empty(2 + 2 * nb, dtype=torch.float64, device="cuda")
    scratch = torch.empty(_lib.lib.espm_binning_sums_scratch(n, ny, nx, nb) // 8, dtype=torch.float64, device="cuda")
    one = torch.empty(4, dtype=torch.float64, device="cuda")
    first = None
    for dtype in (torch.uint8, torch.float32):
        Xd = X8 if dtype == torch.uint8 else X8.to(dtype)
        for layout in ("cm", "pm"):
            X = Xd if layout == "cm" else Xd.t().contiguous()
            name = f"{str(dtype).split('.')[-1]:8s} {layout}"
            xb = X.numel() * X.element_size()
            out = torch.empty((n, gny * gnx) if layout == "cm" else (gny * gnx, n), dtype=torch.float32, device="cuda")
            med, lo, hi = timed(lambda: rebin_call(X, layout, n, ny, nx, (4, 4), out), args.calls)
            ab = xb + out.numel() * 4
            say(f"  rebin (4, 4)  {name}: {med:8.3f} ms ({lo:.3f} - {hi:.3f}); {ab / 1e9:.3f} GB -> {ab / med / 1e6:.0f} GB/s = "
                f"{100 * ab / (med * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")
            del out
            med, lo, hi = timed(lambda: sums_call(X, layout, n, ny, nx, bins, res, scratch), args.calls)
            torch.cuda.synchronize()
            now = res.clone()
            same = "" if first is None else f"; risk minimum as in the first configuration: {int(torch.argmin(risk(now, n, p))) == first}"
            first = int(torch.argmin(risk(now, n, p))) if first is None else first
            read = xb * (nb + 1)
            say(f"  scan of {nb:3d}   {name}: {med:8.3f} ms ({lo:.3f} - {hi:.3f}) = {med / (nb + 1):.3f} ms per pass; X once {xb / 1e9:.3f} GB -> "
                f"{100 * xb / (med * 1e-3) / HBM_PEAK:.2f} % of 8 TB/s; as read, {read / 1e9:.0f} GB -> {read / med / 1e6:.0f} GB/s = "
                f"{100 * read / (med * 1e-3) / HBM_PEAK:.1f} %{same}")
            parts = []
            for b in (1, 2, 4, 8, 16, 64, 256):
                if b > min(ny, nx):
                    continue
                bb = np.ascontiguousarray(np.asarray([(b, b)], dtype=np.int32))
                m1 = timed(lambda: sums_call(X, layout, n, ny, nx, bb, one, scratch), max(5, args.calls // 4))[0]
                parts.append(f"b={b}: {m1:.3f}")
            say(f"      one candidate and the totals, ms: " + ", ".join(parts))
            del X
        del Xd
    say(f"best bin of the scan: {tuple(int(v) for v in bins[first])}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def risk(res, n, p):
    T1, T2, A, C = res[0], res[1], res[2::2], res[3::2]
    return C / (p * n) * p / n + (T2 - T1 - A + C) / (p * n)


if __name__ == "__main__":
    main()
