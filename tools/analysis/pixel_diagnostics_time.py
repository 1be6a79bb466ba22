"""Time of espm_pixel_diagnostics (csrc/mu_diag.hip) at the headline image (2048 channels x 512^2 pixels, k = 5; bench.py's dose of
500 counts per pixel) for 8-bit and fp32 X in both layouts, and at k = 8, against the same quantities from torch in fp64 on the
device (pixel chunks: einsum for F, torch.linalg.inv, the constrained form).

    python tools/analysis/pixel_diagnostics_time.py [--size n,nx,ny] [--runs 3] [--no-baseline] [--out FILE]

X is device-resident (synthetic Poisson counts drawn on the device); every configuration is warmed up once, then timed --runs times
with HIP events around the one launch; min - max is reported.  "bytes" are what the pass has to move once: X in its dtype, D, H, and
the two outputs; the share of the 8 TB/s HBM peak is bytes / time / 8e12 (the pass is bound by fp64 arithmetic, not by memory: one
division, one logarithm per non-zero entry and k + k (k + 1) / 2 FMAs per entry of X).  The kernel's deviance and H_std are compared
with the baseline's on the same image before anything is timed."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from espm_amd import _lib  # noqa: E402
from espm_amd.conf import log_shift  # noqa: E402
from espm_amd.engine import _ptr, _stream, require_gpu  # noqa: E402

COUNTS = 500.0
CODES = {torch.uint8: _lib.DIAG_X_U8, torch.uint16: _lib.DIAG_X_U16, torch.float32: _lib.DIAG_X_F32, torch.float64: _lib.DIAG_X_F64}


def model(n, p, k, g):
    """D (n, k): Gaussian peaks on a floor, columns summing to COUNTS; H (k, p) on the simplex."""
    c = torch.arange(n, device="cuda", dtype=torch.float64)[:, None]
    centres = (torch.arange(k, device="cuda", dtype=torch.float64)[None, :] + 0.5) * n / k
    D = torch.exp(-0.5 * ((c - centres) / (n / (6.0 * k))) ** 2) + 0.05
    D = D * (COUNTS / D.sum(dim=0, keepdim=True))
    H = torch.rand((k, p), generator=g, device="cuda", dtype=torch.float64) + 0.1
    return D.contiguous(), (H / H.sum(dim=0, keepdim=True)).contiguous()


def draw(D, H, g):
    n, p = D.shape[0], H.shape[1]
    X = torch.empty((n, p), dtype=torch.uint8, device="cuda")
    step = max(1, (32 << 20) // p)
    for a in range(0, n, step):   # (row chunks: the fp64 rates of the whole image would be 4 GB)
        X[a:a + step] = torch.poisson(D[a:a + step] @ H, generator=g).clamp_max(255).to(torch.uint8)
    return X


def kernel(X, layout, D, H, simplex, out):
    n, p = (X.shape[0], X.shape[1]) if layout == "cm" else (X.shape[1], X.shape[0])
    _lib.check(_lib.lib.espm_pixel_diagnostics(_ptr(X), CODES[X.dtype], _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM,
                                               int(X.stride(0)), n, p, _ptr(D), _ptr(H), D.shape[1], float(log_shift), int(simplex),
                                               _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream()))


def baseline(X, D, H, simplex, out, chunk=16384):
    """The same quantities with torch, fp64, X (n, p) channel-major, in chunks of pixels."""
    k, p = H.shape
    for a in range(0, p, chunk):
        x = X[:, a:a + chunk].to(torch.float64)
        y = (D @ H[:, a:a + chunk]).clamp_min(log_shift)
        out[0][a:a + chunk] = 2.0 * (torch.xlogy(x, x / y) - x + y).sum(dim=0)
        F = torch.einsum("ci,cj,cp->pij", D, D, 1.0 / y)
        C = torch.linalg.inv(F)
        if simplex:
            u = C.sum(dim=2)
            C = C - u[:, :, None] * u[:, None, :] / u.sum(dim=1)[:, None, None]
        out[1][:, a:a + chunk] = torch.diagonal(C, dim1=1, dim2=2).clamp_min(0).sqrt().T


def timed(fn, runs):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,512,512")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    require_gpu()
    n, nx, ny = (int(v) for v in args.size.split(","))
    p = nx * ny
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"pixel diagnostics, {n} channels x {nx} x {ny} pixels, {COUNTS:.0f} counts per pixel, simplex bound, {torch.cuda.get_device_name(0)}")
    for k in (5, 8):
        g = torch.Generator(device="cuda").manual_seed(k)
        D, H = model(n, p, k, g)
        X8 = draw(D, H, g)
        say(f"k = {k}: {float((X8 != 0).float().mean()):.3f} of the entries are non-zero")
        out = (torch.empty(p, dtype=torch.float64, device="cuda"), torch.empty((k, p), dtype=torch.float64, device="cuda"),
               torch.zeros(1, dtype=torch.int32, device="cuda"))
        ref = (torch.empty_like(out[0]), torch.empty_like(out[1]))
        base = None
        if not args.no_baseline:
            base = timed(lambda: baseline(X8, D, H, True, ref), args.runs)
        for dtype in ((torch.uint8, torch.float32) if k == 5 else (torch.uint8,)):
            Xc = X8 if dtype == torch.uint8 else X8.to(dtype)
            for layout in ("cm", "pm"):
                X = Xc if layout == "cm" else Xc.t().contiguous()
                kernel(X, layout, D, H, True, out)
                torch.cuda.synchronize()
                agree = ""
                if base is not None:
                    agree = (f", max rel. difference from torch: deviance {float(((out[0] - ref[0]).abs() / ref[0].abs().clamp_min(1e-300)).max()):.1e}"
                             f" H_std {float(((out[1] - ref[1]).abs() / ref[1]).max()):.1e}, singular {int(out[2])}")
                lo, hi = timed(lambda: kernel(X, layout, D, H, True, out), args.runs)
                nbytes = X.numel() * X.element_size() + 8 * (D.numel() + H.numel() + out[0].numel() + out[1].numel())
                say(f"  k={k} {str(dtype).split('.')[-1]:8s} {layout}: {lo:8.3f} - {hi:8.3f} ms, {nbytes / 1e9:.3f} GB -> "
                    f"{nbytes / lo / 1e6:.0f} GB/s = {100 * nbytes / (lo * 1e-3) / 8e12:.1f} % of 8 TB/s{agree}")
                del X
            del Xc
        if base is not None:
            say(f"  k={k} torch fp64 baseline (uint8 cm, pixel chunks of 16384): {base[0]:8.3f} - {base[1]:8.3f} ms")
        del X8, D, H, out, ref
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
