"""Time of the residual products (csrc/mu_residual.hip) at the headline image (2048 channels x 512^2 pixels; bench.py's dose of 500
counts per pixel, 8-bit X), both layouts:

  * one pass of the pixel side and of the channel side with 8 dense vectors and the model at k = 5 - every entry read, y formed, one
    fp64 square root and one fp64 division, 9 multiply-adds into the sums;
  * the weighted marginals with 8 all-ones weight vectors at k = 5 on the same image, in the same process: the yardstick - the pass of
    the same geometry that forms the same y and pays an fp64 division and a logarithm per entry, and 24 multiply-adds;
  * a whole ``espm_amd.residuals.svd`` (4 vectors, the default tolerance) of the resident image: two passes per iteration, the
    orthonormalisation of the 8 x p block on the device, the 8 x n block on the host.

    python tools/analysis/residuals_time.py [--size n,ny,nx] [--calls 20] [--out profiles/residuals_time.log]

X is device-resident (synthetic Poisson counts drawn on the device).  Every configuration is warmed up twice, then every one of --calls
calls is timed between its own pair of HIP events; the median is reported (with the minimum and the maximum), as a share of the 8 TB/s
HBM peak on the bytes of X.  Before anything is timed the two layouts are compared bit for bit with each other and the adjoint
u . (E v) = (E^T u) . v is checked."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from espm_amd import _lib, residuals  # noqa: E402
from espm_amd.conf import log_shift  # noqa: E402
from espm_amd.engine import _ptr, _stream, require_gpu  # noqa: E402

from binning_time import HBM_PEAK, timed  # noqa: E402
from marginals_time import marginals_call  # noqa: E402
from pixel_diagnostics_time import CODES, draw, model  # noqa: E402  (the same image as the diagnostics' timings)


def residual_call(X, layout, n, p, side, V, D, H, out, chi2, count, scratch):
    _lib.check(_lib.lib.espm_residual_products(_ptr(X), CODES[X.dtype], _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM,
                                               int(X.stride(0)), n, p, side, _ptr(V), V.shape[0], _ptr(D), _ptr(H), D.shape[1],
                                               float(log_shift), _ptr(out), _ptr(chi2), _ptr(count), _ptr(scratch), scratch.numel(), _stream()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,512,512")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residuals_time.log"))
    args = ap.parse_args()
    require_gpu()
    n, ny, nx = (int(v) for v in args.size.split(","))
    p, k, g = ny * nx, 5, 8
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"residual products, {n} channels x {ny} x {nx} pixels, 500 counts per pixel, 8-bit X, {g} vectors, k = {k}, "
        f"median (min - max) of {args.calls} calls, {torch.cuda.get_device_name(0)}")
    gen = torch.Generator(device="cuda").manual_seed(5)
    D, H = model(n, p, k, gen)
    X = draw(D, H, gen)
    Xt = X.t().contiguous()
    f64 = dict(dtype=torch.float64, device="cuda")
    U, V = torch.randn((g, n), generator=gen, **f64), torch.randn((g, p), generator=gen, **f64)
    ones_n, ones_p = torch.ones((g, n), **f64), torch.ones((g, p), **f64)
    pix, chan = torch.empty((g, p), **f64), torch.empty((g, n), **f64)
    chi_p, chi_n = torch.empty(p, **f64), torch.empty(n, **f64)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(int(_lib.lib.espm_residual_products_scratch(_lib.RESID_CHANNELS, n, p, g)), dtype=torch.uint8, device="cuda")
    mpix, mchan = [torch.empty((g, p), **f64) for _ in range(3)], [torch.empty((g, n), **f64) for _ in range(3)]
    mscratch = torch.empty(int(_lib.lib.espm_weighted_marginals_scratch(_lib.MARG_CHANNELS, n, p, g)), dtype=torch.uint8, device="cuda")

    # correctness first: the two layouts bit for bit, the adjoint, chi2 from both sides
    first = None
    for layout, Xl in (("cm", X), ("pm", Xt)):
        residual_call(Xl, layout, n, p, _lib.RESID_PIXELS, U, D, H, pix, chi_p, count, scratch)
        residual_call(Xl, layout, n, p, _lib.RESID_CHANNELS, V, D, H, chan, chi_n, count, scratch)
        torch.cuda.synchronize()
        got = torch.cat([pix.reshape(-1), chan.reshape(-1), chi_p, chi_n]).clone()
        same = "" if first is None else f"; bit-equal to cm: {bool(torch.equal(got, first))}"
        first = got if first is None else first
        say(f"{layout}: chi2 {float(chi_p.sum()):.9g} (pixels) {float(chi_n.sum()):.9g} (channels), {float(chi_p.sum()) / (n * p):.4f} per entry; "
            f"unmodelled {int(count.item())}{same}")
        del got
    # (the adjoint needs E v for the SAME pair: one vector from each side)
    residual_call(X, "cm", n, p, _lib.RESID_PIXELS, U[:1], D, H, pix[:1], None, None, scratch)
    residual_call(X, "cm", n, p, _lib.RESID_CHANNELS, V[:1], D, H, chan[:1], None, None, scratch)
    torch.cuda.synchronize()
    left, right = float(U[0] @ chan[0]), float(pix[0] @ V[0])
    say(f"adjoint: u . (E v) = {left:.12g}, (E^T u) . v = {right:.12g}, relative gap {abs(left - right) / max(abs(left), 1e-300):.2e}")
    xbytes = X.numel()
    for layout, Xl in (("cm", X), ("pm", Xt)):

        def line(name, t, nbytes):
            med, lo, hi = t
            say(f"  {name:52s} {layout}: {med:8.3f} ms ({lo:.3f} - {hi:.3f}); {nbytes / 1e9:.3f} GB -> {nbytes / med / 1e6:.0f} GB/s = "
                f"{100 * nbytes / (med * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")

        line(f"residual products, pixel side, {g} vectors, k = {k}",
             timed(lambda: residual_call(Xl, layout, n, p, _lib.RESID_PIXELS, U, D, H, pix, chi_p, count, scratch), args.calls), xbytes)
        line(f"marginals, pixel side, {g} x ones, k = {k}",
             timed(lambda: marginals_call(Xl, layout, n, p, _lib.MARG_PIXELS, ones_n, D, H, mpix, mscratch), args.calls), xbytes)
        line(f"residual products, channel side, {g} vectors, k = {k}",
             timed(lambda: residual_call(Xl, layout, n, p, _lib.RESID_CHANNELS, V, D, H, chan, chi_n, count, scratch), args.calls), xbytes)
        line(f"marginals, channel side, {g} x ones, k = {k}",
             timed(lambda: marginals_call(Xl, layout, n, p, _lib.MARG_CHANNELS, ones_p, D, H, mchan, mscratch), args.calls), xbytes)
        line(f"residual products, pixel side, 1 vector, k = {k}",
             timed(lambda: residual_call(Xl, layout, n, p, _lib.RESID_PIXELS, U[:1], D, H, pix[:1], None, None, scratch), args.calls), xbytes)
    # a whole svd of the resident image (the model is right: E is noise, so the iteration runs to max_iter unless the values settle)
    Dh, Hh = D.cpu().numpy(), H.cpu().numpy()
    residuals.svd(X, Dh, Hh, n_vectors=4, max_iter=1)   # (warm-up: the first Gram products and factorisations)
    for layout, Xl in (("cm", X), ("pm", Xt)):
        for max_iter in (10,):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = residuals.svd(Xl, Dh, Hh, n_vectors=4, max_iter=max_iter, layout=layout)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            say(f"  residuals.svd, 4 vectors, {out['n_iter']} iterations ({2 * out['n_iter'] + 1} passes), {layout}: {1e3 * dt:.1f} ms wall; "
                f"s = {out['singular_values'].round(2)}, edge {out['edge']:.1f}, converged {out['converged']}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
