"""Time of the count-splitting kernels (csrc/mu_split.hip) at the headline image (2048 channels x 512^2 pixels; bench.py's dose of 500
counts per pixel, 8-bit X), both layouts: espm_thin_counts (with and without X_b) and espm_split_deviance at 5 components - next to
espm_pixel_diagnostics (5 components) and espm_rebin_pixels (bin (4, 4)) on the same image.

    python tools/analysis/splitting_time.py [--size n,ny,nx] [--calls 20] [--out profiles/splitting_time.log]

X is device-resident (synthetic Poisson counts drawn on the device).  Every configuration is warmed up, then every one of --calls
calls is timed between its own pair of HIP events; the median is reported (with the minimum and the maximum), as a share of the 8 TB/s
HBM peak on the call's ALGORITHMIC bytes: the split reads X once and writes X_a and X_b (three image-sized transfers; two without
X_b), the score reads X once (d, h and the three per-pixel outputs are 0.1 % of it at this size).  Before anything is timed the split is
checked on the whole image - X_a + X_b = X, X_a from the two layouts equal, the total of X_a against q N in its binomial sigma - and the
score's in-sample deviance of X_a against espm_pixel_diagnostics of the materialised X_a."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from espm_amd import _lib, splitting  # noqa: E402
from espm_amd.conf import log_shift  # noqa: E402
from espm_amd.engine import _ptr, _stream, require_gpu  # noqa: E402

from binning_time import HBM_PEAK, rebin_call, timed  # noqa: E402
from pixel_diagnostics_time import CODES, draw, kernel as diag_call, model  # noqa: E402  (the same image as the diagnostics' timings)


def _layout(layout):
    return _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM


def thin_call(X, layout, n, p, thr, seed, xa, xb):
    _lib.check(_lib.lib.espm_thin_counts(_ptr(X), CODES[X.dtype], _layout(layout), int(X.stride(0)), n, p, p, 0, thr, seed, _ptr(xa),
                                         _ptr(xb) if xb is not None else None, int(xa.stride(0)), _stream()))


def deviance_call(X, layout, n, p, thr, seed, D, H, out):
    _lib.check(_lib.lib.espm_split_deviance(_ptr(X), CODES[X.dtype], _layout(layout), int(X.stride(0)), n, p, p, 0, thr, seed, _ptr(D), _ptr(H),
                                            D.shape[1], float(log_shift), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,512,512")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--q", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splitting_time.log"))
    args = ap.parse_args()
    require_gpu()
    n, ny, nx = (int(v) for v in args.size.split(","))
    p, k, seed = ny * nx, 5, 7
    thr, q_eff = splitting.threshold(args.q)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"count splitting, {n} channels x {ny} x {nx} pixels, 500 counts per pixel, 8-bit X, q = {q_eff:.6f}, {k} components, "
        f"median (min - max) of {args.calls} calls, {torch.cuda.get_device_name(0)}")
    g = torch.Generator(device="cuda").manual_seed(5)
    D, H = model(n, p, k, g)
    X = draw(D, H, g)
    total = int(X.sum(dtype=torch.int64))
    say(f"{total / X.numel():.3f} counts per entry, {100 * float((X > 0).sum()) / X.numel():.1f} % of the entries are not zero")
    # correctness first
    Xa, Xb = torch.empty_like(X), torch.empty_like(X)
    thin_call(X, "cm", n, p, thr, seed, Xa, Xb)
    Xt = X.t().contiguous()
    Ta = torch.empty_like(Xt)
    thin_call(Xt, "pm", n, p, thr, seed, Ta, None)
    na = int(Xa.sum(dtype=torch.int64))
    z = (na - q_eff * total) / (total * q_eff * (1 - q_eff)) ** 0.5
    say(f"X_a + X_b = X: {bool(torch.equal(Xa + Xb, X))}; X_a of the two layouts equal: {bool(torch.equal(Ta.t(), Xa))}; total of X_a at "
        f"{z:+.2f} sigma of q N")
    del Ta
    Ha = (H * q_eff).contiguous()   # the model of the training part: the truth at the dose q
    out = [torch.empty(p, dtype=torch.float64, device="cuda"), torch.empty(p, dtype=torch.float64, device="cuda"),
           torch.empty(p, dtype=torch.int64, device="cuda")]
    deviance_call(X, "cm", n, p, thr, seed, D, Ha, out)
    dg = [torch.empty(p, dtype=torch.float64, device="cuda"), torch.empty((k, p), dtype=torch.float64, device="cuda"),
          torch.zeros(1, dtype=torch.int32, device="cuda")]
    diag_call(Xa, "cm", D, Ha, True, dg)
    rel = float(((out[0] - dg[0]).abs() / dg[0]).max())
    say(f"in-sample deviance against espm_pixel_diagnostics of the materialised X_a: max rel. difference {rel:.1e}; held-out counts equal "
        f"{bool(torch.equal(out[2], Xb.sum(dim=0, dtype=torch.int64)))}; deviance per entry: in-sample {float(out[0].sum()) / X.numel():.4f}, "
        f"held out {float(out[1].sum()) / X.numel():.4f}")
    del Xb
    xbytes = X.numel()
    gny, gnx = -(-ny // 4), -(-nx // 4)
    for layout in ("cm", "pm"):
        Xl = X if layout == "cm" else Xt
        A = Xa if layout == "cm" else torch.empty_like(Xt)
        B = torch.empty_like(Xl)

        def line(name, t, nbytes):
            med, lo, hi = t
            say(f"  {name:34s} {layout}: {med:8.3f} ms ({lo:.3f} - {hi:.3f}); {nbytes / 1e9:.3f} GB -> {nbytes / med / 1e6:.0f} GB/s = "
                f"{100 * nbytes / (med * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")

        line("espm_thin_counts (X_a, X_b)", timed(lambda: thin_call(Xl, layout, n, p, thr, seed, A, B), args.calls), 3 * xbytes)
        line("espm_thin_counts (X_a)", timed(lambda: thin_call(Xl, layout, n, p, thr, seed, A, None), args.calls), 2 * xbytes)
        del B
        line("espm_split_deviance", timed(lambda: deviance_call(Xl, layout, n, p, thr, seed, D, Ha, out), args.calls), xbytes)
        line("espm_pixel_diagnostics", timed(lambda: diag_call(Xl, layout, D, Ha, True, dg), args.calls), xbytes)
        rb = torch.empty((n, gny * gnx) if layout == "cm" else (gny * gnx, n), dtype=torch.float32, device="cuda")
        line("espm_rebin_pixels (4, 4)", timed(lambda: rebin_call(Xl, layout, n, ny, nx, (4, 4), rb), args.calls), xbytes + rb.numel() * 4)
        del rb
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
