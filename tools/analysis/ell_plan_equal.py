"""Do the sparse store's launches compute the same bits in two trees?  The record behind gathering their LDS layouts into
csrc/mu_ell_plan.hpp (profiles/ell_plan_equal.log).

    python tools/analysis/ell_plan_equal.py [--root TREE] > OUT.txt      # then diff the OUT.txt of two trees

Imports espm_amd from TREE (default: this tree; its libraries must be built) and runs the rows of tests/ell_plan_cases.py - one per
shape of the fused launch's plan - as tests/test_gpu_ell_plan.py does: three iterations with the loss as the fused launch and as
the two launches, then three H-only iterations on the general path and chained.  Per row and path one line: sha256 of W, of H and
of the history rows."""
import argparse
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ITERS = 3
KW = dict(simplex_H=True, simplex_W=False, lambda_L=0.7, mu=0.05)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:20]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    import ell_plan_cases as ec
    from espm_amd.engine import MUEngine
    for case in ec.CASES:
        os.environ["ESPM_ELL_STREAM_MB"] = "0" if case["stream"] else "1000000"
        X, W0, H0, p = ec.problem(case)

        def line(path, eng):
            torch.cuda.synchronize()
            print(f"{case['id']} {path}: W {digest(eng.get_W())} H {digest(eng.get_H())} history {digest(eng.hist[:ITERS + 1].cpu().numpy())}", flush=True)
        for fused in ("always", False):
            eng = MUEngine(X, case["k"], shape_2d=(1, p), x_store="ell", tile_px=case["pb"] // 2, fused=fused, tol=0.0, max_iter=ITERS + 2, **KW)
            eng.load_state(W0, H0)
            eng.iterate(ITERS, final_loss=True)
            line("fused" if fused else "two launches", eng)
        alt = eng.hpart_alt.data_ptr()
        for chained in (False, True):
            eng.st.hpart_alt = alt if chained else None
            assert eng.h_chain_applies() == chained
            eng.load_state(W0, H0)
            eng.iterate_h(ITERS, final_loss=True)
            line("H-only chained" if chained else "H-only general", eng)


if __name__ == "__main__":
    main()
