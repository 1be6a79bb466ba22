"""Per-iteration time of the fp64 mode (MUEngine(precision="fp64")) at the headline image (2048 channels x 512^2 pixels, k = 5,
simplex_H, lambda_L = 1, 8-bit counts) and at BASELINE configuration 2's size (1980 x 128^2, k = 3, simplex_H).

    python tools/analysis/fp64_iter_time.py [--iters N] [--only headline|c2]

Synthetic Poisson counts drawn on the device; three warm-up iterations, then N iterations between two synchronisations (the
loss of every state is computed, as in a fit)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from espm_amd.engine import MUEngine  # noqa: E402

CASES = {"headline": (2048, 512, 512, 5), "c2": (1980, 128, 128, 3)}


def run(name, iters):
    n, nx, ny, k = CASES[name]
    p = nx * ny
    g = torch.Generator(device="cuda").manual_seed(0)
    D = torch.rand((n, k), generator=g, device="cuda", dtype=torch.float64)
    Ht = -torch.log(torch.rand((k, p), generator=g, device="cuda", dtype=torch.float64))
    Ht /= Ht.sum(dim=0, keepdim=True)
    X = torch.poisson(8.0 * D @ Ht, generator=g).clamp_max(255)
    del Ht
    W0 = (torch.rand((n, k), generator=g, device="cuda", dtype=torch.float64) + 0.1).cpu().numpy()
    H0 = torch.full((k, p), 1.0 / k, dtype=torch.float64).numpy()
    eng = MUEngine(X, k, shape_2d=(nx, ny), lambda_L=1.0, simplex_H=True, simplex_W=False, tol=0.0, max_iter=iters + 8,
                   precision="fp64")
    del X
    eng.load_state(W0, H0)
    eng.iterate(3, final_loss=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.iterate(iters, final_loss=False)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / iters
    loss = eng.history()["loss"][eng.it - 1]
    print(f"fp64 {name}: {n} x {nx}x{ny}, k={k}, store {eng.x_store}: {ms:.3f} ms/iteration over {iters} (loss {loss:.9g})", flush=True)
    del eng
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=sorted(CASES))
    a = ap.parse_args()
    for name in ([a.only] if a.only else ["c2", "headline"]):
        run(name, a.iters)
