#!/usr/bin/env python3
"""Generate f22_explained_intensity.npz from the UNMODIFIED reference: ``espm.utils.get_explained_intensity_W`` (utils.py:396-414) on
a dictionary G, on a square identity G and on a one-component model.  Beside make_golden.py, which it imports for its stand-in of
``exspy``, its path to the reference and its ``save``; make_golden.py itself is not touched and none of its fixtures is rewritten.

    python tests/golden/make_golden_attribution.py

Only DATA is stored: the inputs and the reference's outputs.
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as mg  # noqa: E402  (installs the exspy stand-in and puts the reference on sys.path)
import numpy as np  # noqa: E402
from espm.utils import get_explained_intensity_W  # noqa: E402


def f22():
    rng = np.random.default_rng(22)
    out = {}
    for name, (n, m, k, p) in (("dict", (40, 7, 3, 60)), ("one", (12, 4, 1, 9))):
        G, W, H = rng.random((n, m)), rng.random((m, k)) * 3.0, rng.random((k, p))
        W[1, 0] = 0.0
        out.update({f"{name}_G": G, f"{name}_W": W, f"{name}_H": H, f"{name}_out": get_explained_intensity_W(G, W, H)})
    G, W, H = np.eye(16), rng.random((16, 2)), rng.random((2, 30))
    out.update(eye_G=G, eye_W=W, eye_H=H, eye_out=get_explained_intensity_W(G, W, H))
    mg.save("f22_explained_intensity", **out)


if __name__ == "__main__":
    f22()
