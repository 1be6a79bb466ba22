"""Time of the weighted marginals (csrc/mu_marginals.hip) at the headline image (2048 channels x 512^2 pixels; bench.py's dose of 500
counts per pixel, 8-bit X), both layouts:

  * the pixel side and the channel side with 8 all-ones weight vectors and the model at k = 5 - every entry read, the term formed,
    24 multiply-adds into the sums;
  * the pixel side with 8 windows of 20 channels and no model (k = 0) - the raw line maps, where the skip leaves 160 of 2048 rows;
  * espm_pixel_diagnostics and espm_channel_diagnostics at k = 5 on the same image, in the same process: the yardstick - the pass of
    the same side that forms the same y and term and does more arithmetic per entry (k (k + 1) / 2 = 15 multiply-adds of the Fisher
    information against 3 g = 24 here at g = 8, 3 at g = 1).

    python tools/analysis/marginals_time.py [--size n,ny,nx] [--calls 20] [--out profiles/marginals_time.log]

X is device-resident (synthetic Poisson counts drawn on the device).  Every configuration is warmed up twice, then every one of --calls
calls is timed between its own pair of HIP events; the median is reported (with the minimum and the maximum), as a share of the 8 TB/s
HBM peak on the bytes of X the call has to read (the whole image, or the windows' rows).  Before anything is timed the all-ones sums are
compared bit for bit with the diagnostics' and the two layouts with each other, and the windows' counts with torch's integer sums."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from espm_amd import _lib  # noqa: E402
from espm_amd.conf import log_shift  # noqa: E402
from espm_amd.engine import _ptr, _stream, require_gpu  # noqa: E402

from binning_time import HBM_PEAK, timed  # noqa: E402
from pixel_diagnostics_time import CODES, draw, kernel as pixel_diag_call, model  # noqa: E402  (the same image as the diagnostics' timings)
from spectral_diagnostics_time import kernel as channel_diag_call  # noqa: E402


def marginals_call(X, layout, n, p, side, W, D, H, out, scratch):
    k = 0 if D is None else D.shape[1]
    _lib.check(_lib.lib.espm_weighted_marginals(_ptr(X), CODES[X.dtype], _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM,
                                                int(X.stride(0)), n, p, side, _ptr(W), W.shape[0], _ptr(D), _ptr(H), k, float(log_shift),
                                                _ptr(out[0]), _ptr(out[1] if k else None), _ptr(out[2] if k else None), _ptr(scratch),
                                                scratch.numel(), _stream()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,512,512")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginals_time.log"))
    args = ap.parse_args()
    require_gpu()
    n, ny, nx = (int(v) for v in args.size.split(","))
    p, k, g, width = ny * nx, 5, 8, 20
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"weighted marginals, {n} channels x {ny} x {nx} pixels, 500 counts per pixel, 8-bit X, {g} weight vectors, "
        f"median (min - max) of {args.calls} calls, {torch.cuda.get_device_name(0)}")
    gen = torch.Generator(device="cuda").manual_seed(5)
    D, H = model(n, p, k, gen)
    X = draw(D, H, gen)
    Xt = X.t().contiguous()
    say(f"{float(X.sum(dtype=torch.int64)) / X.numel():.3f} counts per entry, {100 * float((X > 0).sum()) / X.numel():.1f} % of the entries are not zero")
    f64 = dict(dtype=torch.float64, device="cuda")
    ones_n, ones_p = torch.ones((g, n), **f64), torch.ones((g, p), **f64)
    windows = torch.zeros((g, n), **f64)
    starts = [(2 * q + 1) * n // (2 * g) for q in range(g)]   # 8 windows of 20 channels, spread over the spectrum
    for q, a in enumerate(starts):
        windows[q, a:a + width] = 1.0
    pix = [torch.empty((g, p), **f64) for _ in range(3)]
    chan = [torch.empty((g, n), **f64) for _ in range(3)]
    scratch = torch.empty(int(_lib.lib.espm_weighted_marginals_scratch(_lib.MARG_CHANNELS, n, p, g)), dtype=torch.uint8, device="cuda")
    dg = [torch.empty(p, **f64), torch.empty((k, p), **f64), torch.zeros(1, dtype=torch.int32, device="cuda")]
    cg = [torch.empty(n, **f64), torch.empty(n, **f64), torch.empty(n, **f64), torch.empty((n, k * (k + 1) // 2), **f64)]
    cscratch = torch.empty(int(_lib.lib.espm_channel_diagnostics_scratch(n, p, k)) // 8, **f64)

    # correctness first: the diagnostics' sums bit for bit, the two layouts, the windows against integer sums
    first = {}
    for layout, Xl in (("cm", X), ("pm", Xt)):
        marginals_call(Xl, layout, n, p, _lib.MARG_PIXELS, ones_n, D, H, pix, scratch)
        marginals_call(Xl, layout, n, p, _lib.MARG_CHANNELS, ones_p, D, H, chan, scratch)
        pixel_diag_call(Xl, layout, D, H, True, dg)
        channel_diag_call(Xl, layout, D, H, cg, cscratch)
        torch.cuda.synchronize()
        ok_p = all(bool(torch.equal(pix[2][q], dg[0])) for q in (0, g - 1))
        ok_c = all(bool(torch.equal(chan[i][q], cg[j])) for q in (0, g - 1) for i, j in ((0, 1), (1, 2), (2, 0)))
        raw = [torch.empty((g, p), **f64)]
        marginals_call(Xl, layout, n, p, _lib.MARG_PIXELS, windows, None, None, raw, scratch)
        Xc = Xl if layout == "cm" else Xl.t()
        ok_w = all(bool(torch.equal(raw[0][q], Xc[a:a + width].sum(dim=0, dtype=torch.int64).to(torch.float64))) for q, a in enumerate(starts))
        got = torch.cat([t.reshape(-1) for t in pix + chan + raw]).clone()
        same = "" if not first else f"; bit-equal to cm: {bool(torch.equal(got, first['cm']))}"
        first.setdefault(layout, got)
        say(f"{layout}: all-ones deviance maps equal espm_pixel_diagnostics': {ok_p}; all-ones spectra equal espm_channel_diagnostics' "
            f"dev, xsum, ysum: {ok_c}; window counts equal the integer sums: {ok_w}{same}")
        del raw, got
    xbytes = X.numel()
    for layout, Xl in (("cm", X), ("pm", Xt)):

        def line(name, t, nbytes):
            med, lo, hi = t
            say(f"  {name:52s} {layout}: {med:8.3f} ms ({lo:.3f} - {hi:.3f}); {nbytes / 1e9:.3f} GB -> {nbytes / med / 1e6:.0f} GB/s = "
                f"{100 * nbytes / (med * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")

        line(f"marginals, pixel side, {g} x ones, k = {k}",
             timed(lambda: marginals_call(Xl, layout, n, p, _lib.MARG_PIXELS, ones_n, D, H, pix, scratch), args.calls), xbytes)
        line(f"espm_pixel_diagnostics, k = {k}", timed(lambda: pixel_diag_call(Xl, layout, D, H, True, dg), args.calls), xbytes)
        line(f"marginals, channel side, {g} x ones, k = {k}",
             timed(lambda: marginals_call(Xl, layout, n, p, _lib.MARG_CHANNELS, ones_p, D, H, chan, scratch), args.calls), xbytes)
        line(f"espm_channel_diagnostics, k = {k}", timed(lambda: channel_diag_call(Xl, layout, D, H, cg, cscratch), args.calls), xbytes)
        line(f"marginals, pixel side, 1 x ones, k = {k}",
             timed(lambda: marginals_call(Xl, layout, n, p, _lib.MARG_PIXELS, ones_n[:1], D, H, pix, scratch), args.calls), xbytes)
        line(f"marginals, pixel side, {g} windows of {width}, k = 0",
             timed(lambda: marginals_call(Xl, layout, n, p, _lib.MARG_PIXELS, windows, None, None, pix, scratch), args.calls), g * width * p)
        line(f"marginals, pixel side, {g} x ones, k = 0",
             timed(lambda: marginals_call(Xl, layout, n, p, _lib.MARG_PIXELS, ones_n, None, None, pix, scratch), args.calls), xbytes)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
