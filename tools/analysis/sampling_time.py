"""Time of the Poisson-sampling kernels (csrc/mu_sample.hip) at the headline image (2048 channels x 512^2 pixels; bench.py's dose of 500
counts per pixel), both layouts: espm_poisson_sample at 5 components as 8- and 16-bit counts, espm_sample_deviance for one and for four
replicates - and one replicate of NMFEstimator.bootstrap end to end (draw, read-back, refit of a copy) at --boot-size.

    python tools/analysis/sampling_time.py [--size n,ny,nx] [--calls 20] [--boot-size n,ny,nx] [--boot-iter 20] [--out profiles/sampling_time.log]

The model is device-resident (the diagnostics' timings' model).  Every configuration is warmed up, then every one of --calls calls is
timed between its own pair of HIP events; the median is reported (with the minimum and the maximum), and the rate in entries per
second: both kernels are bound by instruction issue (at least one Philox4x32-10 per entry with a fractional rate), not by the bytes
they move - the sampler writes the image once, the deviance moves 0.1 % of that.  Before anything is timed the sample is checked on the
whole image: the two layouts equal, the total against the sum of the rates in its Poisson sigma, the counters zero, and the deviance
kernel's row against espm_pixel_diagnostics of the materialised replicate."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from espm_amd import _lib  # noqa: E402
from espm_amd.conf import log_shift  # noqa: E402
from espm_amd.engine import _ptr, _stream, require_gpu  # noqa: E402

from binning_time import timed  # noqa: E402
from pixel_diagnostics_time import CODES, kernel as diag_call, model  # noqa: E402  (the same model as the diagnostics' timings)


def sample_call(D, H, seed, replicate, X, layout, counts):
    n, k = D.shape
    p = H.shape[1]
    _lib.check(_lib.lib.espm_poisson_sample(_ptr(D), _ptr(H), k, n, p, p, 0, seed, replicate, _ptr(X), CODES[X.dtype],
                                            _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM, int(X.stride(0)), _ptr(counts), _stream()))


def deviance_call(D, H, seed, replicate0, out):
    n, k = D.shape
    p = H.shape[1]
    _lib.check(_lib.lib.espm_sample_deviance(_ptr(D), _ptr(H), k, n, p, p, 0, seed, replicate0, out.shape[0], float(log_shift), _ptr(out), _stream()))


def bootstrap_replicate(size, iters, say):
    """Wall time of one replicate of ``bootstrap``: a fit of ``iters`` iterations of a simulated image first, then two replicates."""
    from espm_amd.estimators import SmoothNMF
    n, ny, nx = size
    p, k = ny * nx, 5
    g = torch.Generator(device="cuda").manual_seed(5)
    D, H = model(n, p, k, g)
    from espm_amd import sampling
    X, info = sampling.sample(D.cpu().numpy(), H.cpu().numpy(), seed=1, dtype=np.uint8)
    est = SmoothNMF(n_components=k, simplex_H=True, simplex_W=False, max_iter=iters, tol=0, no_stop_criterion=True, verbose=0, init="nndsvdar",
                    random_state=0, shape_2d=(ny, nx))
    t0 = time.perf_counter()
    est.fit(X.astype(np.float32))
    t_fit = time.perf_counter() - t0
    t0 = time.perf_counter()
    est.bootstrap(n_boot=2, seed=3, max_iter=iters)
    t_boot = (time.perf_counter() - t0) / 2
    say(f"bootstrap at {n} x {ny} x {nx}, {k} components, {iters} iterations: the fit {t_fit:.2f} s (NNDSVD start), one replicate end to end "
        f"{t_boot:.2f} s (draw, read-back, warm-started refit of a copy); saturated entries of the image {info['saturated']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,512,512")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--boot-size", default="2048,512,512")
    ap.add_argument("--boot-iter", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_time.log"))
    args = ap.parse_args()
    require_gpu()
    n, ny, nx = (int(v) for v in args.size.split(","))
    p, k, seed = ny * nx, 5, 7
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"Poisson sampling, {n} channels x {ny} x {nx} pixels, 500 counts per pixel, {k} components, median (min - max) of {args.calls} calls, "
        f"{torch.cuda.get_device_name(0)}")
    g = torch.Generator(device="cuda").manual_seed(5)
    D, H = model(n, p, k, g)
    counts = torch.empty(2, dtype=torch.int64, device="cuda")
    # correctness first
    X = torch.empty((n, p), dtype=torch.uint8, device="cuda")
    sample_call(D, H, seed, 0, X, "cm", counts)
    Xt = torch.empty((p, n), dtype=torch.uint8, device="cuda")
    sample_call(D, H, seed, 0, Xt, "pm", counts)
    total, expect = int(X.sum(dtype=torch.int64)), float(D.sum(dim=0) @ H.sum(dim=1))
    say(f"{total / X.numel():.3f} counts per entry, {100 * float((X > 0).sum()) / X.numel():.1f} % of the entries are not zero; the two layouts "
        f"equal: {bool(torch.equal(Xt.t(), X))}; total at {(total - expect) / expect ** 0.5:+.2f} sigma of the sum of the rates; counters "
        f"{counts.cpu().tolist()}")
    dev = torch.empty((1, p), dtype=torch.float64, device="cuda")
    deviance_call(D, H, seed, 0, dev)
    dg = [torch.empty(p, dtype=torch.float64, device="cuda"), torch.empty((k, p), dtype=torch.float64, device="cuda"),
          torch.zeros(1, dtype=torch.int32, device="cuda")]
    diag_call(X, "cm", D, H, True, dg)
    say(f"espm_sample_deviance against espm_pixel_diagnostics of the materialised replicate: max rel. difference "
        f"{float(((dev[0] - dg[0]).abs() / dg[0]).max()):.1e}; deviance per entry {float(dev.sum()) / X.numel():.4f}")
    del Xt, dg
    entries = n * p
    for layout in ("cm", "pm"):
        for dtype in (torch.uint8, torch.uint16):
            Xl = torch.empty((n, p) if layout == "cm" else (p, n), dtype=dtype, device="cuda")
            med, lo, hi = timed(lambda: sample_call(D, H, seed, 1, Xl, layout, counts), args.calls)
            say(f"  espm_poisson_sample {str(dtype)[6:]:6s} {layout}: {med:8.3f} ms ({lo:.3f} - {hi:.3f}); {entries / med / 1e6:.1f} G entries/s, "
                f"{Xl.numel() * Xl.element_size() / med / 1e6:.0f} GB/s written")
            del Xl
    for n_rep in (1, 4):
        out = torch.empty((n_rep, p), dtype=torch.float64, device="cuda")
        med, lo, hi = timed(lambda: deviance_call(D, H, seed, 0, out), args.calls)
        say(f"  espm_sample_deviance n_rep = {n_rep}: {med:8.3f} ms ({lo:.3f} - {hi:.3f}); {n_rep * entries / med / 1e6:.1f} G entries/s")
    del X, D, H
    torch.cuda.empty_cache()
    bootstrap_replicate(tuple(int(v) for v in args.boot_size.split(",")), args.boot_iter, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
