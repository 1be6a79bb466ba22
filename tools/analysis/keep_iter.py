#!/usr/bin/env python3
"""The headline image (or ROWS rows of it, COUNTS per pixel, CONFIG=c5: configuration 5) on the sparse store, ITERS fused iterations and
nothing else: what a counter pass of the kept part of streamed lists runs under rocprofv3 (tools/analysis/keep_measure.sh), and a
timing of the same.  The engine reads ESPM_ELL_STREAM_MB, ESPM_ELL_KEEP_MB and ESPM_ELL_KEEP_GROUPS=h:w (espm_amd/engine.py)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from espm_amd import synth  # noqa: E402
from espm_amd.engine import MUEngine  # noqa: E402

ROWS, K = int(os.environ.get("ROWS", "512")), int(os.environ.get("K", "5"))
COUNTS, ITERS = float(os.environ.get("COUNTS", "500")), int(os.environ.get("ITERS", "50"))
C5 = os.environ.get("CONFIG") == "c5"
N_CH, NY, M = (1980, 1024, 17) if C5 else (2048, 512, None)
if C5:
    K = 8
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
prob = synth.make_problem(N_CH, ROWS, NY, K, N=COUNTS, seed=0, row0=0, nx_total=NY, m=M)
X = synth.sample_torch(prob, dev, seed=1000, row0=0)
W0, H0 = synth.random_init(M if C5 else N_CH, K, NY * NY, seed=0, scale=COUNTS / N_CH)
kw = dict(layout="pm", shape_2d=(ROWS, NY), lambda_L=1.0, simplex_H=True, simplex_W=False, tol=0.0, max_iter=2 * ITERS + 20, device=dev)
if C5:
    kw.update(G=prob["G"], mu=0.05)
eng = MUEngine(X, K, **kw)
del X
eng.load_state(W0, H0[:, :ROWS * NY])
eng.iterate(ITERS // 2, final_loss=False)
torch.cuda.synchronize()
t0 = time.perf_counter()
eng.iterate(ITERS - ITERS // 2, final_loss=False)
torch.cuda.synchronize()
us = (time.perf_counter() - t0) / (ITERS - ITERS // 2) * 1e6
st = eng.st
kept = ""
if hasattr(st, "ell_keep_h"):
    from espm_amd import ell as _ell
    kb = getattr(eng, "keep_bytes", None)
    if kb is not None:
        kh = sum(kb[0][j] for j in _ell.keep_indices(st.ell_keep_h, len(kb[0])))
        kwb = sum(kb[1][j] for j in _ell.keep_indices(st.ell_keep_w, len(kb[1])))
        kept = (f", kept {st.ell_keep_h} of {len(kb[0])} list groups per tile ({kh / 1e6:.1f} of {sum(kb[0]) / 1e6:.1f} MB), "
                f"{st.ell_keep_w} of {len(kb[1])} channel groups ({kwb / 1e6:.1f} of {sum(kb[1]) / 1e6:.1f} MB)")
print(f"rows {ROWS} counts {COUNTS:g} k {K}: lists {eng.x_bytes / 1e6:.1f} MB, ell_stream {st.ell_stream}{kept}: {us:.1f} us / iteration", flush=True)
