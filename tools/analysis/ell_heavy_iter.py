#!/usr/bin/env python3
"""Heavy elements of the sparse store (include/espm_mu.h, ell_hv_*) at the headline geometry: per-iteration time of
  (a) the image as generated,  (b) one element set to 1000,  (c) a fraction of the non-zero elements set to counts in 256 .. 4000,
each on the sparse store and (c) also on the forced fp32 store, interleaved over rounds, medians.  Also the set-up time of each engine
(the store's build included) and, with --crossover, more fractions on the sparse store to place store.ELL_MAX_HEAVY_FRACTION.
--profile FRAC: only the sparse store at that fraction, for a rocprofv3 --kernel-trace --stats run.  JSON lines on stdout."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from espm_amd import synth
from espm_amd.engine import MUEngine

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--fractions", default="0.001,0.01,0.05")
ap.add_argument("--crossover", default="")
ap.add_argument("--profile", type=float, default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
n, nx, ny, k = 2048, 512, 512, 5
prob = synth.make_problem(n, nx, ny, k, N=500.0, seed=0)
X0 = synth.sample_torch(prob, dev, seed=1000)            # (p, n) f32 counts, the bench's image
W0, H0 = synth.random_init(n, k, nx * ny, seed=0, scale=500.0 / n)
W0, H0 = torch.from_numpy(W0).to(dev, torch.float32), torch.from_numpy(H0).to(dev, torch.float32)
nz = torch.nonzero(X0.view(-1)).flatten()
perm = torch.randperm(nz.numel(), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
vals = torch.randint(256, 4001, (nz.numel(),), device=dev, generator=torch.Generator(device=dev).manual_seed(6)).float()


def image(kind):
    if kind == "a":
        return X0
    X = X0.clone()
    if kind == "b":
        X.view(-1)[nz[0]] = 1000.0
    else:
        m = int(float(kind) * nz.numel())
        X.view(-1)[nz[perm[:m]]] = vals[:m]
    return X


def run(kind, store):
    X = image(kind)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng = MUEngine(X, k, layout="pm", shape_2d=(nx, ny), lambda_L=1.0, simplex_H=True, simplex_W=False, tol=0.0,
                   max_iter=args.iters + 60, device=dev, x_store=store, autotune=False)
    torch.cuda.synchronize()
    setup_ms = 1e3 * (time.perf_counter() - t0)
    del X
    eng.load_state(W0, H0)
    eng.iterate(30, final_loss=False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    eng.iterate(args.iters, final_loss=False)
    e1.record()
    torch.cuda.synchronize()
    us = 1e3 * e0.elapsed_time(e1) / args.iters
    out = dict(kind=kind, store=eng.x_store, heavy=int(eng.st.ell_hv_n) if eng.x_store == "ell" else None, us_per_iter=round(us, 2),
               setup_ms=round(setup_ms, 1))
    del eng
    torch.cuda.empty_cache()
    return out


if args.profile is not None:
    print(json.dumps(run(str(args.profile), "ell")), flush=True)
    sys.exit(0)

legs = [("a", "ell"), ("b", "ell")]
for f in args.fractions.split(","):
    legs += [(f, "ell"), (f, "f32")]
for f in filter(None, args.crossover.split(",")):
    legs.append((f, "ell"))
results = {}
for r in range(args.rounds):
    for leg in legs:
        res = run(*leg)
        results.setdefault(leg, []).append(res)
        print(json.dumps(dict(round=r, **res)), flush=True)
for leg, rs in results.items():
    us = sorted(x["us_per_iter"] for x in rs)
    setup = sorted(x["setup_ms"] for x in rs)
    print(json.dumps(dict(summary=True, kind=leg[0], store=rs[0]["store"], heavy=rs[0]["heavy"], median_us=us[len(us) // 2],
                          median_setup_ms=setup[len(setup) // 2], rounds=len(rs))), flush=True)
