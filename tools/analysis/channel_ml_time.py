"""Time of one lockstep pass of the channel ML (espm_spectra_ml_pass_batch + espm_channel_ml_step, csrc/mu_channel_ml.hip) against the
batched pass alone, and of ``channel_ml.presence`` and ``channel_ml.intervals`` end to end, at the headline image (2048 channels x
512^2 pixels, k = 5, 8-bit X; bench.py's dose of 500 counts per pixel).

    python tools/analysis/channel_ml_time.py [--size n,nx,ny] [--k 5] [--batches 1,5,10] [--runs 10] [--calls 5] [--out FILE]

1. The lockstep pass.  X is device-resident synthetic Poisson counts.  For every B of --batches the models are the fit's own: B = 1
   the free-scale model, otherwise pinned models (component b mod k held at 0.8 or 1.2 of its true spectrum).  A window starts every
   problem afresh from a perturbed start (espm_channel_ml_step with start = 1, outside the timed part) and then times --calls x
   (pass, step) between two HIP events at tol = 1e-12, so that no problem retires inside the window (the live problems after it are
   reported); the batched pass alone, over the same models with every flag set, is timed in the window next to it, --runs times,
   INTERLEAVED.  Reported: the medians and min - max, and what the step adds to the pass.
2. End to end.  ``presence`` (the full fit, then the k reduced fits as one batch) and ``intervals`` (all 2 k ends of every channel
   as one batch) from the default start: wall time with the upload of H and the read-backs, passes, evaluations, convergence."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from espm_amd import _lib, channel_ml  # noqa: E402
from espm_amd.conf import log_shift  # noqa: E402
from espm_amd.engine import _ptr, _stream, require_gpu  # noqa: E402

from pixel_diagnostics_time import CODES, draw, model  # noqa: E402  (the same image as the diagnostics)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,512,512")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--batches", default="1,5,10")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    require_gpu()
    n, nx, ny = (int(v) for v in args.size.split(","))
    p, k = nx * ny, args.k
    nt = k * (k + 1) // 2
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"channel ML, {n} channels x {nx} x {ny} pixels, k = {k}, u8 X, 500 counts per pixel, {args.runs} interleaved windows of "
        f"{args.calls} lockstep passes, {torch.cuda.get_device_name(0)}")
    g = torch.Generator(device="cuda").manual_seed(k)
    D, H = model(n, p, k, g)
    X = draw(D, H, g)
    f64 = dict(dtype=torch.float64, device="cuda")
    s = np.ascontiguousarray(H.sum(dim=1).cpu().numpy())
    xsum = X.sum(dim=1, dtype=torch.float64)
    image = (_ptr(X), CODES[X.dtype], _lib.LAYOUT_CM, int(X.stride(0)), n, p)
    mask = (1 << k) - 1
    for B in (int(v) for v in args.batches.split(",")):
        pins = np.array([-1] if B == 1 else [b % k for b in range(B)], dtype=np.int32)
        start = torch.stack([D * (0.5 + torch.rand((n, k), generator=g, **f64)) for _ in range(B)]).contiguous()
        t = torch.stack([D[:, max(int(j), 0)] * (0.8 if b % 2 == 0 else 1.2) for b, j in enumerate(pins)]).contiguous()
        d = start.clone()
        dev_in, ysum, q, tri = (torch.zeros(sh, **f64) for sh in ((B, n), (B, n), (B, n, k), (B, n, nt)))
        un = torch.zeros(B, dtype=torch.int64, device="cuda")
        scratch = torch.empty(_lib.lib.espm_spectra_ml_pass_batch_scratch(n, p, k, B) // 8, **f64)
        state = torch.zeros((B, 2 * k + _lib.CML_STATE_EXTRA, n), **f64)
        dev, gap, slope = (torch.zeros((B, n), **f64) for _ in range(3))
        passes = torch.zeros((B, n), dtype=torch.int32, device="cuda")
        done = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
        active, ones = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.ones(B, dtype=torch.uint8, device="cuda")
        live = torch.zeros(B, dtype=torch.int64, device="cuda")

        def pass_(flags):
            _lib.check(_lib.lib.espm_spectra_ml_pass_batch(*image, _ptr(d), _ptr(H), k, B, _ptr(flags), float(log_shift), _ptr(dev_in),
                                                           _ptr(ysum), _ptr(q), _ptr(tri), _ptr(un), _ptr(scratch), scratch.numel() * 8,
                                                           _stream()))

        def step(first):
            _lib.check(_lib.lib.espm_channel_ml_step(n, k, B, first, _ptr(dev_in), _ptr(q), _ptr(tri), _ptr(xsum),
                                                     s.ctypes.data_as(ctypes.c_void_p), mask, pins.ctypes.data_as(ctypes.c_void_p), _ptr(t),
                                                     1e-12, _ptr(d), _ptr(state), state.numel() * 8, _ptr(dev), _ptr(gap), _ptr(slope),
                                                     _ptr(passes), _ptr(done), _ptr(active), _ptr(live), _stream()))

        def window(lockstep):
            d.copy_(start)
            done.zero_()
            step(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                if lockstep:
                    pass_(active)
                    step(0)
                else:
                    pass_(ones)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.calls

        for lockstep in (True, False):   # warm-up: code objects, the first launches
            window(lockstep)
        tl, tp, left = [], [], []
        for _ in range(args.runs):
            tl.append(window(True))
            left.append(int(live.sum().item()))
            tp.append(window(False))
        ml, mp = statistics.median(tl), statistics.median(tp)
        say(f"  B = {B:2d} ({'free-scale' if B == 1 else 'pinned'}): lockstep pass {ml:.3f} ms (median; {min(tl):.3f} - {max(tl):.3f}), "
            f"batched pass alone {mp:.3f} ms ({min(tp):.3f} - {max(tp):.3f}): the step adds {ml - mp:+.3f} ms = {100 * (ml / mp - 1):+.2f} % "
            f"({mp / B:.3f} ms a model and pass); live after a window {min(left)} - {max(left)} of {B * n} problems")
        del start, d, dev_in, ysum, q, tri, scratch, state
    torch.cuda.empty_cache()

    Hh = H.cpu().numpy()
    for name, fn in (("presence", channel_ml.presence), ("intervals", channel_ml.intervals)):
        for run in range(2):   # (the second: nothing left to load or to allocate for the first time)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(X, Hh)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            if name == "presence":
                say(f"presence() run {run}: {total:.3f} s; full fit {int(res['n_pass'][0].max())} passes at most, the {k} reduced fits (one batch) "
                    f"{int(res['n_pass'][1:].max())} at most; all converged: {bool(res['converged'].all())}; lr == 0 at "
                    f"{int((res['lr'] == 0).sum())} of {res['lr'].size} entries, p < 0.01 at {int((res['pvalue'] < 0.01).sum())}")
            else:
                say(f"intervals() run {run}: {total:.3f} s for {2 * k} ends per channel; at most {int(res['n_eval'].max())} evaluations and "
                    f"{int(res['n_pass'].max())} passes an end (median {int(np.median(res['n_eval']))} / {int(np.median(res['n_pass']))}); all found: "
                    f"{bool(res['converged'].all())}; lower == 0 at {int((res['lower'] == 0).sum())} of {res['lower'].size} entries")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
