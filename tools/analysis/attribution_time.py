"""Time of the count-attribution kernels (csrc/mu_attrib.hip) at the headline image (2048 channels x 512^2 pixels; bench.py's dose of 500
counts per pixel, 8-bit X), 5 components, both layouts: espm_attribute_expected (its three launches together) and espm_assign_counts -
next to espm_pixel_diagnostics and espm_thin_counts on the same image, in the same process, as the scale.

    python tools/analysis/attribution_time.py [--size n,ny,nx] [--calls 20] [--out profiles/attribution_time.log]

X is device-resident (synthetic Poisson counts drawn on the device).  Every configuration is warmed up twice, then every one of --calls
calls is timed between its own pair of HIP events; the median is reported (with the minimum and the maximum), as a share of the 8 TB/s
HBM peak on the call's ALGORITHMIC bytes: the expected attribution reads X twice (a pass per side; d, h, the outputs and the scratch are
2 % of it at this size), the random one reads X once and writes k images.  Before anything is timed the identities are checked on the
whole image: the parts add up to X, the parts of the two layouts are equal, their totals sit at the expected attribution within the
multinomial sigma, sum_j pixel_counts = counts, sum_c D o R = sum_p pixel_counts, and the two layouts of the expected attribution give
the same bits."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from espm_amd import _lib, splitting  # noqa: E402
from espm_amd.conf import log_shift  # noqa: E402
from espm_amd.engine import _ptr, _stream, require_gpu  # noqa: E402

from binning_time import HBM_PEAK, timed  # noqa: E402
from pixel_diagnostics_time import CODES, draw, kernel as diag_call, model  # noqa: E402  (the same image as the diagnostics' timings)
from splitting_time import _layout, thin_call  # noqa: E402


def expected_call(X, layout, n, p, D, H, out, scratch):
    _lib.check(_lib.lib.espm_attribute_expected(_ptr(X), CODES[X.dtype], _layout(layout), int(X.stride(0)), n, p, _ptr(D), _ptr(H), D.shape[1],
                                                float(log_shift), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(scratch), scratch.numel(),
                                                _stream()))


def assign_call(X, layout, n, p, D, H, seed, parts, cnt):
    _lib.check(_lib.lib.espm_assign_counts(_ptr(X), CODES[X.dtype], _layout(layout), int(X.stride(0)), n, p, p, 0, _ptr(D), _ptr(H), D.shape[1],
                                           seed, _ptr(parts), int(parts.stride(0)), int(parts.stride(1)), _ptr(cnt), _stream()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,512,512")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attribution_time.log"))
    args = ap.parse_args()
    require_gpu()
    n, ny, nx = (int(v) for v in args.size.split(","))
    p, k, seed = ny * nx, 5, 7
    thr, _ = splitting.threshold(0.8)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"count attribution, {n} channels x {ny} x {nx} pixels, 500 counts per pixel, 8-bit X, {k} components, "
        f"median (min - max) of {args.calls} calls, {torch.cuda.get_device_name(0)}")
    g = torch.Generator(device="cuda").manual_seed(5)
    D, H = model(n, p, k, g)
    X = draw(D, H, g)
    Xt = X.t().contiguous()
    total = int(X.sum(dtype=torch.int64))
    say(f"{total / X.numel():.3f} counts per entry, {100 * float((X > 0).sum()) / X.numel():.1f} % of the entries are not zero")

    def outputs():
        return [torch.empty((k, p), dtype=torch.float64, device="cuda"), torch.empty((n, k), dtype=torch.float64, device="cuda"),
                torch.empty(p, dtype=torch.int64, device="cuda")]

    scratch = torch.empty(int(_lib.lib.espm_attribute_expected_scratch(n, p, k)), dtype=torch.uint8, device="cuda")
    # correctness first
    ex, et = outputs(), outputs()
    expected_call(X, "cm", n, p, D, H, ex, scratch)
    expected_call(Xt, "pm", n, p, D, H, et, scratch)
    same = all(bool(torch.equal(a, b)) for a, b in zip(ex, et))
    counts = ex[2].to(torch.float64)
    gap_p = float(((ex[0].sum(dim=0) - counts).abs() / counts.clamp_min(1)).max())
    by_channel, by_pixel = (D * ex[1]).sum(dim=0), ex[0].sum(dim=1)
    gap_t = float(((by_channel - by_pixel).abs() / by_pixel).max())
    say(f"expected: the two layouts give the same bits: {same}; counts exact: {bool(torch.equal(ex[2], X.sum(dim=0, dtype=torch.int64)))}; "
        f"sum_j pixel_counts = counts to {gap_p:.1e} (rel., worst pixel); sum_c D o R = sum_p pixel_counts to {gap_t:.1e}")
    cnt = torch.empty(1, dtype=torch.int64, device="cuda")
    parts = torch.empty((k, n, p), dtype=X.dtype, device="cuda")
    assign_call(X, "cm", n, p, D, H, seed, parts, cnt)
    adds_up = all(bool(torch.equal(parts[:, a:a + 256].sum(dim=0, dtype=torch.int32), X[a:a + 256].to(torch.int32))) for a in range(0, n, 256))
    tot = torch.stack([parts[i].sum(dtype=torch.int64) for i in range(k)]).to(torch.float64)
    z = (tot - by_pixel) / by_pixel.sqrt()   # (the multinomial variance of a total is below its mean)
    parts_t = torch.empty((k, p, n), dtype=X.dtype, device="cuda")
    assign_call(Xt, "pm", n, p, D, H, seed, parts_t, cnt)
    both = all(bool(torch.equal(parts_t[i].t(), parts[i])) for i in range(k))
    say(f"assign: the parts add up to X: {adds_up}; the parts of the two layouts are equal: {both}; invalid entries: {int(cnt.item())}; "
        "totals against the expected attribution, in units of sqrt(mean) (an upper bound of sigma): " + ", ".join(f"{float(v):+.2f}" for v in z))
    say("explained counts ratio: " + ", ".join(f"{float(v) / total:.4f}" for v in by_pixel))
    xbytes = X.numel()
    dg = [torch.empty(p, dtype=torch.float64, device="cuda"), torch.empty((k, p), dtype=torch.float64, device="cuda"),
          torch.zeros(1, dtype=torch.int32, device="cuda")]
    for layout in ("cm", "pm"):
        Xl = X if layout == "cm" else Xt
        Pl = parts if layout == "cm" else parts_t

        def line(name, t, nbytes):
            med, lo, hi = t
            say(f"  {name:34s} {layout}: {med:8.3f} ms ({lo:.3f} - {hi:.3f}); {nbytes / 1e9:.3f} GB -> {nbytes / med / 1e6:.0f} GB/s = "
                f"{100 * nbytes / (med * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s")

        line("espm_attribute_expected", timed(lambda: expected_call(Xl, layout, n, p, D, H, ex, scratch), args.calls), 2 * xbytes)
        line(f"espm_assign_counts (k = {k})", timed(lambda: assign_call(Xl, layout, n, p, D, H, seed, Pl, cnt), args.calls), (1 + k) * xbytes)
        line("espm_pixel_diagnostics", timed(lambda: diag_call(Xl, layout, D, H, True, dg), args.calls), xbytes)
        A, B = torch.empty_like(Xl), torch.empty_like(Xl)
        line("espm_thin_counts (X_a, X_b)", timed(lambda: thin_call(Xl, layout, n, p, thr, seed, A, B), args.calls), 3 * xbytes)
        del A, B
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
