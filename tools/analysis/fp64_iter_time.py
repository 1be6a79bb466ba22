"""Per-iteration time of the fp64 mode (MUEngine(precision="fp64")) at the headline image (2048 channels x 512^2 pixels, k = 5,
simplex_H, lambda_L = 1, 8-bit counts) and at BASELINE configuration 2's size (1980 x 128^2, k = 3, simplex_H).

    python tools/analysis/fp64_iter_time.py [--iters N] [--only headline|c2] [--store auto|sparse|u8|f64[,...]] [--density D[,...]]
                                            [--empty-channels N] [--repeat R]

Synthetic Poisson counts drawn on the device; three warm-up iterations, then N iterations between two synchronisations (the
loss of every state is computed, as in a fit).  --density: the share of non-zero entries (default: the dense 8-count image);
--store: the engine's x_store, several to time them on ONE image in one process, interleaved --repeat times (sparse against
dense: the spread between the repeats is the run-to-run noise); --empty-channels: that many channels of the image emptied (the
log_shift fill: the dense path lands on the f64 store)."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from espm_amd.engine import MUEngine  # noqa: E402

CASES = {"headline": (2048, 512, 512, 5), "c2": (1980, 128, 128, 3)}


def image(name, density, empty_channels):
    """The case's synthetic count image as a uint8 device tensor (n, p), and a start (W0, H0)."""
    n, nx, ny, k = CASES[name]
    p = nx * ny
    g = torch.Generator(device="cuda").manual_seed(0)
    D = torch.rand((n, k), generator=g, device="cuda", dtype=torch.float64)
    Ht = -torch.log(torch.rand((k, p), generator=g, device="cuda", dtype=torch.float64))
    Ht /= Ht.sum(dim=0, keepdim=True)
    dose = 8.0 if density is None else -2.0 * math.log1p(-density)   # (D Ht has mean 1/2; the share of non-zeros comes out near it)
    X = torch.empty((n, p), dtype=torch.uint8, device="cuda")
    step = max(1, (32 << 20) // p)
    for a in range(0, n, step):   # (in row chunks: the fp64 rates of the whole image would be 4 GB at the headline size)
        X[a:a + step] = torch.poisson(dose * D[a:a + step] @ Ht, generator=g).clamp_max(255).to(torch.uint8)
    del Ht
    if empty_channels:
        X[torch.linspace(0, n - 1, empty_channels, device="cuda").long()] = 0
    W0 = (torch.rand((n, k), generator=g, device="cuda", dtype=torch.float64) + 0.1).cpu().numpy()
    H0 = torch.full((k, p), 1.0 / k, dtype=torch.float64).numpy()
    return X, W0, H0


def run(name, iters, X, W0, H0, store):
    n, nx, ny, k = CASES[name]
    eng = MUEngine(X, k, shape_2d=(nx, ny), lambda_L=1.0, simplex_H=True, simplex_W=False, tol=0.0, max_iter=iters + 8,
                   precision="fp64", x_store=store)
    eng.load_state(W0, H0)
    eng.iterate(3, final_loss=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.iterate(iters, final_loss=False)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / iters
    loss = eng.history()["loss"][eng.it - 1]
    print(f"fp64 {name}: {n} x {nx}x{ny}, k={k}, store {eng.x_store}: {ms:.3f} ms/iteration over {iters} (loss {loss:.15g})", flush=True)
    del eng
    torch.cuda.empty_cache()
    return ms


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=sorted(CASES))
    ap.add_argument("--store", default="auto")
    ap.add_argument("--density", default="")
    ap.add_argument("--empty-channels", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=1)
    a = ap.parse_args()
    for name in ([a.only] if a.only else ["c2", "headline"]):
        for d in ([float(v) for v in a.density.split(",")] if a.density else [None]):
            X, W0, H0 = image(name, d, a.empty_channels)
            print(f"fp64 {name}: density asked {d}, non-zero share {int(torch.count_nonzero(X)) / X.numel():.4f}, {a.empty_channels} channels emptied", flush=True)
            times = {st: [] for st in a.store.split(",")}
            for _ in range(a.repeat):
                for st in times:
                    times[st].append(run(name, a.iters, X, W0, H0, st))
            for st, ts in times.items():
                print(f"fp64 {name} density {d} x_store={st}: min {min(ts):.3f} max {max(ts):.3f} ms/iteration over {len(ts)} runs", flush=True)
            del X
            torch.cuda.empty_cache()
