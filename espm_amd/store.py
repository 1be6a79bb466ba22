"""Which store an image goes on (the fp32 engine's x_store='auto' / 'ell'): what has to be known about X, and the decision as a
function of those facts alone - plain Python values, no tensor, no device (tests/test_store_choice_cpu.py).  MUEngine scans X
(engine.py, _scan_x), calls ``choose_store`` and lets the ranks agree on its two codes."""
from __future__ import annotations

from typing import NamedTuple, Optional

from . import _lib
from .ell import lds_bytes_h

ELL_MAX_DENSITY = 0.5   # the sparse count store is chosen (x_store='auto') when at most this fraction of X is non-zero: measured crossover with the dense 8-bit store at k = 5: 42 % non-zero 312 vs 394 us, 58 % 410 vs 399 us
ELL_MAX_HEAVY_FRACTION = 0.1    # ... and at most this fraction of its non-zero counts is above 255 (heavy elements): measured at k = 5, 10 % 564 vs 796 us on the f32 store, 20 % 988 vs 796 (NOTEBOOK.md section 11)
ELL_MAX_N = 16384       # channels the sparse store's lists index
CODES = ("f32", "bf16", "u8", "ell")   # the store codes, ordered so that the ranks agree on their minimum


class XFacts(NamedTuple):
    """What the caller of MUEngine already knows about X exactly as handed over (espm_amd/estimators/base.py: the scans that ride
    behind the upload): the passes over X that would establish the same in the engine (9 ms at the headline size) are skipped.
    One GPU, no lines to fill."""
    nonneg: bool     # no entry is negative
    sum_x: float
    is_int: bool     # every entry is an integer
    x_max: float
    nnz: int

    @property
    def is_count(self):
        return bool(self.is_int and self.x_max <= 255)


class StoreFacts(NamedTuple):
    """What the store choice asks of X.  A fact whose pass over X the earlier ones make pointless is None (n_heavy: 0)."""
    is_int: bool
    x_max: Optional[float] = None        # of integer data
    n_heavy: int = 0                     # counts of ELL_HEAVY_MIN and more, of integer data with 255 < x_max <= ELL_HEAVY_MAX
    bf16_exact: Optional[bool] = None    # of data that are not counts <= 255
    nnz: Optional[int] = None            # of counts <= 255 and of data with heavy elements


def choose_store(n, p, k, x_store, facts, *, h_rule=0, bregman=False, pg_gamma_w=0.0, heavy_on=True):
    """The store of an (n channels, p pixels) image with the StoreFacts ``facts`` under x_store 'auto' or 'ell', k components:
    (code, dense_code, note, warn).  code indexes CODES; dense_code is the store a rank with heavy elements falls back to when
    another rank cannot take the sparse store (bf16 or f32; 3 where the rank has no say).  note: why sparse count data did not get
    the sparse store (MUEngine.x_store_note), else None; warn: the note deserves a RuntimeWarning.

    u8 / ell: integer counts <= 255.  ell (non-zero entries only) when at most ELL_MAX_DENSITY of the entries are non-zero and the
    GW table fits in LDS.  Integer counts above 255 (up to 2^24) are the sparse store's heavy elements (include/espm_mu.h, ell_hv_*)
    where the fit's path has them wired in; heavy_on=False (ESPM_ELL_HEAVY=0) restores the choice without them."""
    n_heavy = facts.n_heavy if heavy_on else 0
    code = 2 if facts.is_int and facts.x_max <= 255 else (1 if facts.bf16_exact else 0)
    dense_code = code if n_heavy else 3
    if code != 2 and not n_heavy:
        return code, dense_code, None, False
    heavy_why = None   # why this fit's path cannot take heavy elements
    if n_heavy:
        if int(h_rule) != 0:
            heavy_why = "the heavy elements are wired in for the default H rule only"
        elif bregman:
            heavy_why = "the heavy elements are not wired into the Bregman variant"
        elif float(pg_gamma_w) > 0:
            heavy_why = "the heavy elements are not wired into the projected-gradient W step"
    # (k first: a build is not asked for a component count it has no sparse kernels for)
    lds = lds_bytes_h((n + 7) // 8 * 8, k) if k <= _lib.WIDE_MAX_K else None
    fits = lds is not None and n <= ELL_MAX_N and lds <= _lib.ELL_LDS_MAX
    nnz = facts.nnz
    sparse = float(nnz) <= ELL_MAX_DENSITY * (n * p)
    light = n_heavy <= ELL_MAX_HEAVY_FRACTION * nnz
    if fits and heavy_why is None and (x_store == "ell" or (sparse and light)):
        return 3, dense_code, None, False
    if not sparse:
        return code, dense_code, None, False
    if n_heavy:
        dense = CODES[code]
        if heavy_why is not None:
            note = f"sparse count data with {n_heavy} counts above 255, but {heavy_why}: the dense {dense} store is used"
        elif not fits:
            note = (f"sparse count data with {n_heavy} counts above 255, but the sparse store is built for up to "
                    f"{_lib.WIDE_MAX_K} components and n <= {ELL_MAX_N} with a G W table that fits in LDS (n={n}, "
                    f"k={k}): the dense {dense} store is used")
        else:
            note = (f"sparse count data, but {n_heavy} of its {nnz} non-zero counts are above 255 (more than "
                    f"{ELL_MAX_HEAVY_FRACTION:.0%}, where the sparse store stops paying): the dense {dense} store is used")
        return code, dense_code, note, False
    if k > _lib.WIDE_MAX_K:
        return code, dense_code, (f"sparse count data, but the sparse store is built for up to {_lib.WIDE_MAX_K} components (k={k}: a table row of "
                                  "32 floats leaves a workgroup's LDS no room): the dense 8-bit store is used, both contractions on the matrix cores"), False
    # not silently (missing 3): sparse count data that the sparse store would take - about 3 x the dense store's
    # rate at 20 % non-zero entries - but whose G W table does not fit a workgroup's LDS next to a tile's numerators
    # (rows of 12 / 16 floats from 9 / 13 components on: 16 components stop at 2048 channels, 12 at 2896)
    return code, dense_code, (f"sparse count data, but the sparse store's table for n={n}, k={k} needs "
                              f"{lds} bytes of LDS (limit {_lib.ELL_LDS_MAX}): the dense 8-bit store is used, "
                              "about 3 x slower per iteration at this density"), True
