"""The fp32 engine's choice of a store for X (espm_amd/store.py: choose_store) and the scan that feeds it (engine._scan_x), without a
GPU: the choice is a function of plain values, the scan is tensor plumbing that runs on host tensors.  The engines built on the
choice are exercised by tests/test_gpu_estimator.py and tests/test_gpu_ell_heavy.py.

The expected values of CASES were taken from the decision as it stood inline in MUEngine.__init__ before it became a function (its
block lifted into a script and run on these inputs), not from choose_store."""
import pytest
import torch

P = 600   # pixels of every case; densities are nnz / (n * P), ELL_MAX_DENSITY = 0.5 of it is n * 300 entries

# (what, n, k, x_store, StoreFacts (is_int, x_max, n_heavy, bf16_exact, nnz) as the scan fills them, keywords off their defaults,
#  (code, dense_code, note, warn));  (k, n) "at the LDS limit": the pairs of test_gpu_estimator.py::test_sparse_store_at_the_160_kb_limits
#  (13 and 15 components have room for more than 2048 channels: one channel block further is still sparse there)
CASES = [
    ('counts at 20 %', 160, 3, 'auto', (True, 7.0, 0, None, 19200), {},
     (3, 3, None, False)),
    ('counts at the density limit', 160, 3, 'auto', (True, 7.0, 0, None, 48000), {},
     (3, 3, None, False)),
    ('counts just above the density limit', 160, 3, 'auto', (True, 255.0, 0, None, 48001), {},
     (2, 3, None, False)),
    ('counts at 80 %', 160, 3, 'auto', (True, 7.0, 0, None, 76800), {},
     (2, 3, None, False)),
    ('sparse counts, 17 components', 2048, 17, 'auto', (True, 7.0, 0, None, 245760), {},
     (2, 3, "sparse count data, but the sparse store is built for up to 16 components (k=17: a table row of 32 floats leaves a workgroup's LDS no room): the dense 8-bit store is used, both contractions on the matrix cores", False)),
    ('dense counts, 17 components', 2048, 17, 'auto', (True, 7.0, 0, None, 983040), {},
     (2, 3, None, False)),
    ('sparse counts, table beyond the LDS', 2120, 14, 'auto', (True, 7.0, 0, None, 254400), {},
     (2, 3, "sparse count data, but the sparse store's table for n=2120, k=14 needs 164352 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('dense counts, table beyond the LDS', 2120, 14, 'auto', (True, 7.0, 0, None, 1017600), {},
     (2, 3, None, False)),
    ('sparse counts, more channels than the lists index', 16392, 3, 'auto', (True, 7.0, 0, None, 1967040), {},
     (2, 3, "sparse count data, but the sparse store's table for n=16392, k=3 needs 274560 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('sparse counts at the LDS limit', 2048, 13, 'auto', (True, 7.0, 0, None, 245760), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 2056, 13, 'auto', (True, 7.0, 0, None, 246720), {},
     (3, 3, None, False)),
    ('sparse counts at the LDS limit', 2048, 15, 'auto', (True, 7.0, 0, None, 245760), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 2056, 15, 'auto', (True, 7.0, 0, None, 246720), {},
     (3, 3, None, False)),
    ('sparse counts at the LDS limit', 2048, 16, 'auto', (True, 7.0, 0, None, 245760), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 2056, 16, 'auto', (True, 7.0, 0, None, 246720), {},
     (2, 3, "sparse count data, but the sparse store's table for n=2056, k=16 needs 164352 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('sparse counts at the LDS limit', 2896, 12, 'auto', (True, 7.0, 0, None, 347520), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 2904, 12, 'auto', (True, 7.0, 0, None, 348480), {},
     (2, 3, "sparse count data, but the sparse store's table for n=2904, k=12 needs 163968 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('sparse counts at the LDS limit', 3024, 9, 'auto', (True, 7.0, 0, None, 362880), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 3032, 9, 'auto', (True, 7.0, 0, None, 363840), {},
     (2, 3, "sparse count data, but the sparse store's table for n=3032, k=9 needs 163968 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('sparse counts at the LDS limit', 4608, 8, 'auto', (True, 7.0, 0, None, 552960), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 4616, 8, 'auto', (True, 7.0, 0, None, 553920), {},
     (2, 3, "sparse count data, but the sparse store's table for n=4616, k=8 needs 164096 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('sparse counts at the LDS limit', 9216, 4, 'auto', (True, 7.0, 0, None, 1105920), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 9224, 4, 'auto', (True, 7.0, 0, None, 1106880), {},
     (2, 3, "sparse count data, but the sparse store's table for n=9224, k=4 needs 163968 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('heavy, light and sparse', 160, 3, 'auto', (True, 60000.0, 192, True, 19200), {},
     (3, 1, None, False)),
    ('heavy, light and sparse, not exact in bf16', 160, 3, 'auto', (True, 60000.0, 192, False, 19200), {},
     (3, 0, None, False)),
    ('heavy at the heavy fraction', 160, 3, 'auto', (True, 60000.0, 1920, False, 19200), {},
     (3, 0, None, False)),
    ('heavy just above the heavy fraction', 160, 3, 'auto', (True, 60000.0, 1921, False, 19200), {},
     (0, 0, 'sparse count data, but 1921 of its 19200 non-zero counts are above 255 (more than 10%, where the sparse store stops paying): the dense f32 store is used', False)),
    ('heavy, light, at the density limit', 160, 3, 'auto', (True, 60000.0, 5, False, 48000), {},
     (3, 0, None, False)),
    ('heavy, light, dense', 160, 3, 'auto', (True, 60000.0, 5, True, 76800), {},
     (1, 1, None, False)),
    ('heavy, h_rule 1', 160, 3, 'auto', (True, 60000.0, 5, False, 19200), {'h_rule': 1},
     (0, 0, 'sparse count data with 5 counts above 255, but the heavy elements are wired in for the default H rule only: the dense f32 store is used', False)),
    ('heavy, h_rule 2, dense', 160, 3, 'auto', (True, 60000.0, 5, False, 76800), {'h_rule': 2},
     (0, 0, None, False)),
    ('heavy, Bregman', 160, 3, 'auto', (True, 60000.0, 5, True, 19200), {'bregman': True},
     (1, 1, 'sparse count data with 5 counts above 255, but the heavy elements are not wired into the Bregman variant: the dense bf16 store is used', False)),
    ('heavy, projected-gradient W step', 160, 3, 'auto', (True, 60000.0, 5, False, 19200), {'pg_gamma_w': 2.0},
     (0, 0, 'sparse count data with 5 counts above 255, but the heavy elements are not wired into the projected-gradient W step: the dense f32 store is used', False)),
    ('heavy, h_rule 1 and Bregman', 160, 3, 'auto', (True, 60000.0, 5, False, 19200), {'h_rule': 1, 'bregman': True},
     (0, 0, 'sparse count data with 5 counts above 255, but the heavy elements are wired in for the default H rule only: the dense f32 store is used', False)),
    ('heavy, heavy elements switched off', 160, 3, 'auto', (True, 60000.0, 0, True, None), {'heavy_on': False},
     (1, 3, None, False)),
    ('heavy, 17 components', 2048, 17, 'auto', (True, 60000.0, 5, False, 245760), {},
     (0, 0, 'sparse count data with 5 counts above 255, but the sparse store is built for up to 16 components and n <= 16384 with a G W table that fits in LDS (n=2048, k=17): the dense f32 store is used', False)),
    ('heavy, table beyond the LDS', 2120, 14, 'auto', (True, 60000.0, 5, True, 254400), {},
     (1, 1, 'sparse count data with 5 counts above 255, but the sparse store is built for up to 16 components and n <= 16384 with a G W table that fits in LDS (n=2120, k=14): the dense bf16 store is used', False)),
    ('heavy at the largest heavy count', 160, 3, 'auto', (True, 16777216.0, 5, False, 19200), {},
     (3, 0, None, False)),
    ('a count above the largest heavy count', 160, 3, 'auto', (True, 16777218.0, 0, False, None), {},
     (0, 3, None, False)),
    ('not integer, exact in bf16', 160, 3, 'auto', (False, None, 0, True, None), {},
     (1, 3, None, False)),
    ('not integer, not exact in bf16', 160, 3, 'auto', (False, None, 0, False, None), {},
     (0, 3, None, False)),
    ('counts at 20 %', 160, 3, 'ell', (True, 7.0, 0, None, 19200), {},
     (3, 3, None, False)),
    ('counts at the density limit', 160, 3, 'ell', (True, 7.0, 0, None, 48000), {},
     (3, 3, None, False)),
    ('counts just above the density limit', 160, 3, 'ell', (True, 255.0, 0, None, 48001), {},
     (3, 3, None, False)),
    ('counts at 80 %', 160, 3, 'ell', (True, 7.0, 0, None, 76800), {},
     (3, 3, None, False)),
    ('sparse counts, 17 components', 2048, 17, 'ell', (True, 7.0, 0, None, 245760), {},
     (2, 3, "sparse count data, but the sparse store is built for up to 16 components (k=17: a table row of 32 floats leaves a workgroup's LDS no room): the dense 8-bit store is used, both contractions on the matrix cores", False)),
    ('dense counts, 17 components', 2048, 17, 'ell', (True, 7.0, 0, None, 983040), {},
     (2, 3, None, False)),
    ('sparse counts, table beyond the LDS', 2120, 14, 'ell', (True, 7.0, 0, None, 254400), {},
     (2, 3, "sparse count data, but the sparse store's table for n=2120, k=14 needs 164352 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('dense counts, table beyond the LDS', 2120, 14, 'ell', (True, 7.0, 0, None, 1017600), {},
     (2, 3, None, False)),
    ('sparse counts, more channels than the lists index', 16392, 3, 'ell', (True, 7.0, 0, None, 1967040), {},
     (2, 3, "sparse count data, but the sparse store's table for n=16392, k=3 needs 274560 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('sparse counts at the LDS limit', 2048, 13, 'ell', (True, 7.0, 0, None, 245760), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 2056, 13, 'ell', (True, 7.0, 0, None, 246720), {},
     (3, 3, None, False)),
    ('sparse counts at the LDS limit', 2048, 15, 'ell', (True, 7.0, 0, None, 245760), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 2056, 15, 'ell', (True, 7.0, 0, None, 246720), {},
     (3, 3, None, False)),
    ('sparse counts at the LDS limit', 2048, 16, 'ell', (True, 7.0, 0, None, 245760), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 2056, 16, 'ell', (True, 7.0, 0, None, 246720), {},
     (2, 3, "sparse count data, but the sparse store's table for n=2056, k=16 needs 164352 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('sparse counts at the LDS limit', 2896, 12, 'ell', (True, 7.0, 0, None, 347520), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 2904, 12, 'ell', (True, 7.0, 0, None, 348480), {},
     (2, 3, "sparse count data, but the sparse store's table for n=2904, k=12 needs 163968 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('sparse counts at the LDS limit', 3024, 9, 'ell', (True, 7.0, 0, None, 362880), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 3032, 9, 'ell', (True, 7.0, 0, None, 363840), {},
     (2, 3, "sparse count data, but the sparse store's table for n=3032, k=9 needs 163968 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('sparse counts at the LDS limit', 4608, 8, 'ell', (True, 7.0, 0, None, 552960), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 4616, 8, 'ell', (True, 7.0, 0, None, 553920), {},
     (2, 3, "sparse count data, but the sparse store's table for n=4616, k=8 needs 164096 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('sparse counts at the LDS limit', 9216, 4, 'ell', (True, 7.0, 0, None, 1105920), {},
     (3, 3, None, False)),
    ('sparse counts one channel block past the LDS limit', 9224, 4, 'ell', (True, 7.0, 0, None, 1106880), {},
     (2, 3, "sparse count data, but the sparse store's table for n=9224, k=4 needs 163968 bytes of LDS (limit 163840): the dense 8-bit store is used, about 3 x slower per iteration at this density", True)),
    ('heavy, light and sparse', 160, 3, 'ell', (True, 60000.0, 192, True, 19200), {},
     (3, 1, None, False)),
    ('heavy, light and sparse, not exact in bf16', 160, 3, 'ell', (True, 60000.0, 192, False, 19200), {},
     (3, 0, None, False)),
    ('heavy at the heavy fraction', 160, 3, 'ell', (True, 60000.0, 1920, False, 19200), {},
     (3, 0, None, False)),
    ('heavy just above the heavy fraction', 160, 3, 'ell', (True, 60000.0, 1921, False, 19200), {},
     (3, 0, None, False)),
    ('heavy, light, at the density limit', 160, 3, 'ell', (True, 60000.0, 5, False, 48000), {},
     (3, 0, None, False)),
    ('heavy, light, dense', 160, 3, 'ell', (True, 60000.0, 5, True, 76800), {},
     (3, 1, None, False)),
    ('heavy, h_rule 1', 160, 3, 'ell', (True, 60000.0, 5, False, 19200), {'h_rule': 1},
     (0, 0, 'sparse count data with 5 counts above 255, but the heavy elements are wired in for the default H rule only: the dense f32 store is used', False)),
    ('heavy, h_rule 2, dense', 160, 3, 'ell', (True, 60000.0, 5, False, 76800), {'h_rule': 2},
     (0, 0, None, False)),
    ('heavy, Bregman', 160, 3, 'ell', (True, 60000.0, 5, True, 19200), {'bregman': True},
     (1, 1, 'sparse count data with 5 counts above 255, but the heavy elements are not wired into the Bregman variant: the dense bf16 store is used', False)),
    ('heavy, projected-gradient W step', 160, 3, 'ell', (True, 60000.0, 5, False, 19200), {'pg_gamma_w': 2.0},
     (0, 0, 'sparse count data with 5 counts above 255, but the heavy elements are not wired into the projected-gradient W step: the dense f32 store is used', False)),
    ('heavy, h_rule 1 and Bregman', 160, 3, 'ell', (True, 60000.0, 5, False, 19200), {'h_rule': 1, 'bregman': True},
     (0, 0, 'sparse count data with 5 counts above 255, but the heavy elements are wired in for the default H rule only: the dense f32 store is used', False)),
    ('heavy, heavy elements switched off', 160, 3, 'ell', (True, 60000.0, 0, True, None), {'heavy_on': False},
     (1, 3, None, False)),
    ('heavy, 17 components', 2048, 17, 'ell', (True, 60000.0, 5, False, 245760), {},
     (0, 0, 'sparse count data with 5 counts above 255, but the sparse store is built for up to 16 components and n <= 16384 with a G W table that fits in LDS (n=2048, k=17): the dense f32 store is used', False)),
    ('heavy, table beyond the LDS', 2120, 14, 'ell', (True, 60000.0, 5, True, 254400), {},
     (1, 1, 'sparse count data with 5 counts above 255, but the sparse store is built for up to 16 components and n <= 16384 with a G W table that fits in LDS (n=2120, k=14): the dense bf16 store is used', False)),
    ('heavy at the largest heavy count', 160, 3, 'ell', (True, 16777216.0, 5, False, 19200), {},
     (3, 0, None, False)),
    ('a count above the largest heavy count', 160, 3, 'ell', (True, 16777218.0, 0, False, None), {},
     (0, 3, None, False)),
    ('not integer, exact in bf16', 160, 3, 'ell', (False, None, 0, True, None), {},
     (1, 3, None, False)),
    ('not integer, not exact in bf16', 160, 3, 'ell', (False, None, 0, False, None), {},
     (0, 3, None, False)),
]


@pytest.fixture(scope="module")
def store():
    import __graft_entry__ as ge
    ge.build()
    from espm_amd import store
    return store


@pytest.mark.parametrize("what,n,k,x_store,facts,kw,expected", CASES, ids=[f"{c[3]}-{c[0]}-n{c[1]}-k{c[2]}" for c in CASES])
def test_choose_store(store, what, n, k, x_store, facts, kw, expected):
    assert store.choose_store(n, P, k, x_store, store.StoreFacts(*facts), **kw) == expected


def test_choice_needs_no_more_than_the_scan_gives(store):
    """Facts the scan leaves out (None) are not read: data that are neither counts nor hold heavy elements need no non-zero count."""
    f = store.StoreFacts(is_int=True, x_max=float((1 << 24) + 2), n_heavy=0, bf16_exact=False, nnz=None)
    assert store.choose_store(160, P, 3, "auto", f) == (0, 3, None, False)
    f = store.StoreFacts(is_int=False, x_max=None, n_heavy=0, bf16_exact=True, nnz=None)
    assert store.choose_store(160, P, 3, "ell", f, h_rule=2, bregman=True, pg_gamma_w=1.0) == (1, 3, None, False)
    # heavy elements counted but switched off: as if there were none
    f = store.StoreFacts(is_int=True, x_max=300.0, n_heavy=4, bf16_exact=True, nnz=None)
    assert store.choose_store(160, P, 3, "auto", f, heavy_on=False) == (1, 3, None, False)


def test_thresholds(store):
    from espm_amd import _lib
    assert (store.ELL_MAX_DENSITY, store.ELL_MAX_HEAVY_FRACTION, store.ELL_MAX_N) == (0.5, 0.1, 16384)
    assert (_lib.WIDE_MAX_K, _lib.ELL_LDS_MAX, _lib.ELL_HEAVY_MIN, _lib.ELL_HEAVY_MAX) == (16, 160 * 1024, 256, 1 << 24)
    assert store.CODES == ("f32", "bf16", "u8", "ell")


def test_x_facts(store):
    f = store.XFacts(nonneg=True, sum_x=12.0, is_int=True, x_max=255.0, nnz=7)
    assert f.is_count and not f._replace(x_max=256.0).is_count and not f._replace(is_int=False).is_count


def _counts(seed=0, shape=(50, 40)):
    return torch.poisson(torch.full(shape, 0.3, dtype=torch.float64), generator=torch.Generator().manual_seed(seed))


def test_scan_takes_the_passes_that_have_a_say(store):
    """Which facts the scan establishes (a fact it leaves at None is a pass over X not made), and their values."""
    from espm_amd.engine import _scan_x
    X = _counts()
    nnz = int((X != 0).sum())
    assert _scan_x(X) == store.StoreFacts(True, float(X.max()), 0, None, nnz)                      # counts: no bf16 round trip
    H = X.clone()
    H[3, 4], H[7, 0], H[9, 9] = 256, 70000, 1 << 24
    nnz_h = int((H != 0).sum())
    assert _scan_x(H) == store.StoreFacts(True, float(1 << 24), 3, False, nnz_h)
    assert _scan_x(H.float()) == store.StoreFacts(True, float(1 << 24), 3, False, nnz_h)
    assert _scan_x(H, heavy_on=False) == store.StoreFacts(True, float(1 << 24), 0, False, None)    # no heavy count, no non-zero count
    H[9, 9] += 2
    assert _scan_x(H) == store.StoreFacts(True, float((1 << 24) + 2), 0, False, None)              # beyond the heavy elements' range
    B = X.clone()
    B[0, 0] = 300                                                                                 # (300 is a bf16 value: 75 * 4)
    assert _scan_x(B) == store.StoreFacts(True, 300.0, 1, True, nnz + int(X[0, 0] == 0))
    assert _scan_x(X + 0.5) == store.StoreFacts(False, None, 0, True, None)                        # not integer: no maximum
    assert _scan_x(X + 0.3) == store.StoreFacts(False, None, 0, False, None)


def test_scan_trusts_the_callers_facts(store):
    """With the caller's XFacts, integrality, maximum and non-zero count are taken from them (here: facts that X does not bear out)."""
    from espm_amd.engine import _scan_x
    X = _counts(1)
    known = store.XFacts(nonneg=True, sum_x=float(X.sum()), is_int=True, x_max=9.0, nnz=123)
    assert _scan_x(X, known) == store.StoreFacts(True, 9.0, 0, None, 123)
    H = X.clone()
    H[2, 2] = 1001
    known = store.XFacts(nonneg=True, sum_x=float(H.sum()), is_int=True, x_max=1001.0, nnz=321)
    assert _scan_x(H, known) == store.StoreFacts(True, 1001.0, 1, False, 321)                      # (the heavy count and the round trip are the scan's own)
    assert _scan_x(H, known._replace(is_int=False)) == store.StoreFacts(False, None, 0, False, None)
