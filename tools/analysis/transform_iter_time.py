"""Per-iteration time of an H-only fit (transform) three ways, on the headline image (2048 channels x 512^2 pixels, k = 5, simplex_H,
lambda_L = 1) on the sparse and on the 8-bit store and at BASELINE configuration 2's size (1980 x 128^2, k = 3, sparse store).

    python tools/analysis/transform_iter_time.py [--iters N] [--only headline_ell|headline_u8|c2] [--repeat R]

Legs, interleaved --repeat times in ONE process on one image (the spread between the repeats is the run-to-run noise):
  (a) full iterations with fixed_W = W through MUEngine.iterate: the only way before espm_mu_iterate_h - the W half-step runs and its
      result is overwritten;
  (b) MUEngine.iterate_h on the general path (espm_mu_step_h + espm_mu_h_finalize per iteration: hpart_alt = NULL, the engine's default);
  (c) MUEngine.iterate_h chained: one launch per iteration (hpart_alt set, what ESPM_H_CHAIN=1 does).
Synthetic Poisson counts drawn on the device; three warm-up iterations, then N iterations between two synchronisations."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from espm_amd.engine import MUEngine  # noqa: E402

CASES = {"headline_ell": (2048, 512, 512, 5, "ell", 0.2), "headline_u8": (2048, 512, 512, 5, "u8", None), "c2": (1980, 128, 128, 3, "ell", 0.2)}


def image(name):
    n, nx, ny, k, store, density = CASES[name]
    p = nx * ny
    g = torch.Generator(device="cuda").manual_seed(0)
    D = torch.rand((n, k), generator=g, device="cuda", dtype=torch.float64)
    Ht = -torch.log(torch.rand((k, p), generator=g, device="cuda", dtype=torch.float64))
    Ht /= Ht.sum(dim=0, keepdim=True)
    dose = 8.0 if density is None else -2.0 * math.log1p(-density)   # (D Ht has mean 1/2)
    X = torch.empty((n, p), dtype=torch.float32, device="cuda")
    step = max(1, (32 << 20) // p)
    for a in range(0, n, step):
        X[a:a + step] = torch.poisson(dose * D[a:a + step] @ Ht, generator=g).clamp_max(255).to(torch.float32)
    del Ht
    W0 = (torch.rand((n, k), generator=g, device="cuda", dtype=torch.float64) + 0.1).cpu().numpy()
    H0 = torch.full((k, p), 1.0 / k, dtype=torch.float64).numpy()
    return X, W0, H0


def timed(fn, iters):
    fn(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(iters)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / iters


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--only", choices=sorted(CASES))
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    for name in ([a.only] if a.only else ["c2", "headline_ell", "headline_u8"]):
        n, nx, ny, k, store, _ = CASES[name]
        X, W0, H0 = image(name)
        kw = dict(shape_2d=(nx, ny), lambda_L=1.0, simplex_H=True, simplex_W=False, tol=0.0, max_iter=(a.iters + 4) * a.repeat * 2 + 8, x_store=store)
        full = MUEngine(X, k, fixed_W=W0, **kw)
        honly = MUEngine(X, k, **kw) if hasattr(MUEngine, "iterate_h") else None
        del X
        full.load_state(W0, H0)
        legs = {"a: full iterations, fixed_W": lambda m: full.iterate(m, final_loss=False)}
        if honly is not None:
            honly.load_state(W0, H0)
            alt = honly.hpart_alt.data_ptr()

            def general(m):
                honly.st.hpart_alt = None
                honly.iterate_h(m, final_loss=False)

            def chained(m):
                honly.st.hpart_alt = alt
                assert honly.h_chain_applies()
                honly.iterate_h(m, final_loss=False)
            legs["b: iterate_h, general path"] = general
            legs["c: iterate_h, chained"] = chained
        print(f"transform {name}: {n} x {nx}x{ny}, k={k}, store {full.x_store}, H tiles of {full.st.tile_px} pixels, {a.iters} iterations per run", flush=True)
        times = {leg: [] for leg in legs}
        for _ in range(a.repeat):
            for leg, fn in legs.items():
                times[leg].append(timed(fn, a.iters))
        for leg, ts in times.items():
            print(f"transform {name} ({leg}): min {min(ts):.1f} max {max(ts):.1f} us/iteration over {len(ts)} runs [{' '.join(f'{t:.1f}' for t in ts)}]", flush=True)
        del full, honly, legs
        torch.cuda.empty_cache()
