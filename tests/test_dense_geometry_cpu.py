"""The `expect` column of tests/dense_geometry_cases.py against the loops' own arithmetic, and the completeness of the table - without a
GPU.  (tests/test_gpu_dense_geometry.py asserts the geometry again on the engines' states and runs the rows.)"""
import dense_geometry_cases as dg

ROWS = dg.CASES


def _p(row):
    return row["shape"][0] * row["shape"][1]


def _by_family(name):
    return [r for r in ROWS if r["family"] == name]


def test_ring_shape_on_hand_counted_loops():
    """The helper itself, on loops counted by hand from mu_h_kernel.hpp:688-739 / mu_w_kernel.hpp:80-128."""
    assert dg.ring_shape(32, 8, 2) == (1, 0, 0, 0)        # 4 groups: one trip of 2 NBUF groups
    assert dg.ring_shape(31, 8, 2) == (0, 2, 1, 7)        # 3 groups: no trip, the ring's two, one plain
    assert dg.ring_shape(43, 8, 2) == (1, 1, 0, 3)
    assert dg.ring_shape(63, 8, 2) == (1, 2, 1, 7)
    assert dg.ring_shape(65, 8, 2) == (2, 0, 0, 1)
    assert dg.ring_shape(7, 8, 2) == (0, 0, 0, 7)         # ngroups == 0: the ring is not entered
    assert dg.ring_shape(24, 4, 3) == (1, 0, 0, 0)
    assert dg.ring_shape(23, 4, 3) == (0, 3, 2, 3)
    assert dg.ring_shape(47, 4, 3) == (1, 3, 2, 3)
    assert dg.ring_shape(48, 4, 3) == (2, 0, 0, 0)
    assert dg.ring_shape(16, 4, 3) == (0, 3, 1, 0)        # the 16-pixel blocks every small image gets: the steady-state loop never runs
    assert dg.ring_shape(38, 8, 0) == (0, 0, 4, 6)
    assert dg.ring_shape(37, 4, 0) == (0, 0, 9, 1)


def test_ids_are_unique_and_rows_are_well_formed():
    ids = [r["id"] for r in ROWS]
    assert len(ids) == len(set(ids))
    for r in ROWS:
        p = _p(r)
        assert p < 1024 and r["n"] <= 520, r["id"]
        assert r["store"] in dg.STORES and r["tile_px"] in (128, 256) and r["rule"] in ("kl", "l2", "hq", "pg"), r["id"]
        xt = r["x_tile"] or r["tile_px"]
        assert xt % r["tile_px"] == 0 and 512 % xt == 0, r["id"]                      # check_state's conditions
        assert r["k"] <= 16 or r["tile_px"] == 128, r["id"]                             # the 17..32 build has 128-pixel tiles only
        assert r["k"] <= 16 or r["fused"] or r["store"] == "f32", r["id"]               # ... and vector kernels for the fp32 store only
        assert r["rule"] == "kl" or r["store"] == "f32", r["id"]
        assert not (r["opt"]["simplex_H"] and r["opt"]["simplex_W"]), r["id"]
        if dg.matrix_core_row(r):   # (the bound against the vector twin is absolute: H on the simplex)
            assert r["opt"]["simplex_H"], r["id"]
        if r["w_blocks"] is not None:
            assert 1 <= r["w_blocks"] <= dg.default_w_blocks(p), r["id"]


def test_every_row_produces_the_loop_shapes_it_expects():
    for r in ROWS:
        e, p = r["expect"], _p(r)
        assert e["why"], r["id"]
        if e["loop"] == "h":
            assert not dg.h_on_matrix_cores(r), r["id"]
            assert sorted(set(dg.h_wave_shapes(r["n"], r["tile_px"]))) == e["shapes"], r["id"]
        elif e["loop"] == "h_mfma":
            assert dg.h_on_matrix_cores(r), r["id"]
            assert dg.mfma_h_trips(r["n"]) == e["trips"] and dg.mfma_h_guarded_rows(r["n"], r["store"]) == e["guarded"], r["id"]
        elif e["loop"] == "w":
            assert not dg.w_on_matrix_cores(r), r["id"]
            assert sorted(set(dg.w_block_shapes(p, r["w_blocks"], r["store"]))) == e["shapes"], r["id"]
        elif e["loop"] == "w_mfma":
            assert dg.w_on_matrix_cores(r), r["id"]
            gpb, blocks = dg.mfma_w_groups(p, dg.w_geometry(p, r["w_blocks"])[1])
            assert (gpb, blocks) == (e["gpb"], e["blocks"]), r["id"]
        else:
            raise AssertionError(r["id"])
        if "x_terms" in e:
            assert dg.x_tile_terms(p, r["tile_px"], r["x_tile"]) == e["x_terms"] and min(e["x_terms"]) >= 1, r["id"]


def test_w_blocks_arithmetic():
    """ppb and nblk_w as the table claims them are what MUEngine(w_blocks=) computes: ppb = ceil(p / w_blocks), nblk_w = ceil(p / ppb) -
    and the kernel's own ppb, ceil(p / nblk_w) (mu_common.hpp: make_w_args), is the same number."""
    rows = _by_family("Wring") + _by_family("Wmfma-gpb")
    assert rows
    for r in rows:
        p, e = _p(r), r["expect"]
        ppb = (p + r["w_blocks"] - 1) // r["w_blocks"]
        nblk = (p + ppb - 1) // ppb
        assert (ppb, nblk) == (e["ppb"], e["nblk_w"]) == dg.w_geometry(p, r["w_blocks"]), r["id"]
        assert (p + nblk - 1) // nblk == ppb, r["id"]
    for p in range(16, 1024):          # (for every image the table could hold: the two ppb agree, the last block is not empty)
        for wb in range(1, dg.default_w_blocks(p) + 1):
            ppb, nblk = dg.w_geometry(p, wb)
            assert (p + nblk - 1) // nblk == ppb and (nblk - 1) * ppb < p


def test_h256_holds_every_component_count_on_every_store():
    rows = _by_family("H256")
    for store in dg.STORES:
        vec = {r["k"] for r in rows if r["store"] == store and not dg.h_on_matrix_cores(r)}
        mf = {r["k"] for r in rows if r["store"] == store and dg.h_on_matrix_cores(r)}
        assert vec == set(range(1, 17)) and mf == {13, 14, 15, 16}, store
        opts = [r["opt"] for r in rows if r["store"] == store]
        assert any(o["simplex_H"] and o["lambda_L"] > 0 and o["mu"] for o in opts) and any(o["simplex_W"] for o in opts) and \
            any(not o["simplex_H"] and not o["simplex_W"] for o in opts), store
        assert {r["k"] for r in rows if r["store"] == store and r["fit"]} == {1, 5, 8, 9, 13, 16}
        assert sum(1 for r in rows if r["store"] == store and r["w_step"]) >= 1
    assert all(r["tile_px"] == 256 and r["shape"] == (19, 23) and r["n"] == 150 for r in rows)


def test_the_alternate_rules_have_their_256_pixel_rows():
    rows = _by_family("H256-rules")
    for rule in ("l2", "hq", "pg"):
        assert {r["k"] for r in rows if r["rule"] == rule} >= {1, 5, 8, 9, 16}
    assert all(r["tile_px"] == 256 and r["store"] == "f32" for r in rows)


def _classes_shown(loop, nbuf, rows):
    """{class name: ids of the rows with a wave / block of that class} for one (kernel family, NBUF) pair."""
    shown = {name: [] for name in dg.REQUIRED_RING[(loop, nbuf)]}
    for r in rows:
        shapes = dg.h_wave_shapes(r["n"], r["tile_px"]) if loop == "h" else dg.w_block_shapes(_p(r), r["w_blocks"], r["store"])
        for name, pred in dg.REQUIRED_RING[(loop, nbuf)].items():
            if any(pred(s) for s in shapes):
                shown[name].append(r["id"])
    return shown


def test_the_rows_cover_every_class_of_every_ring():
    """Every class the issue lists, for every (kernel family, NBUF) pair - and, for the rings, for every kernel instance (store and
    component count) of the H128-ring and Wring families: the loops are templates over K with static ring indices."""
    hrows = [r for r in ROWS if r["expect"]["loop"] == "h"]
    for nbuf, tile in ((2, 128), (0, 256)):
        shown = _classes_shown("h", nbuf, [r for r in hrows if r["tile_px"] == tile])
        assert all(shown.values()), shown
    ring = _by_family("H128-ring")
    for inst in sorted({(r["store"], r["k"]) for r in ring}):
        shown = _classes_shown("h", 2, [r for r in ring if (r["store"], r["k"]) == inst])
        assert all(shown.values()), (inst, shown)
    assert {(r["store"], r["k"]) for r in ring} == {(s, k) for s in dg.STORES for k in (3, 8, 12)} | {("f32", 20)}
    wrows = _by_family("Wring")
    for nbuf, stores in ((3, ("u8",)), (0, ("bf16", "f32"))):
        shown = _classes_shown("w", nbuf, [r for r in wrows if r["store"] in stores])
        assert all(shown.values()), shown
    assert {r["store"] for r in wrows} == set(dg.STORES)
    for k in (2, 5, 8, 12):
        mine = [r for r in wrows if r["store"] == "u8" and r["k"] == k]
        shown = _classes_shown("w", 3, mine)
        assert shown["one trip, a full drain, plain groups and singles"] and shown["two trips"], (k, shown)
        # a shorter last block of another class than the blocks before it
        assert any(dg.w_block_shapes(_p(r), r["w_blocks"], "u8")[-1] != dg.w_block_shapes(_p(r), r["w_blocks"], "u8")[0] for r in mine), k
        assert all(r["fused"] == (k <= 8) for r in mine)
    assert {r["k"] for r in wrows if r["expect"]["shapes"] == [(1, 0, 0, 0)]} >= {5, 12}     # 8 and 4 channels per lane


def test_the_matrix_core_loops_have_their_rows():
    trips = _by_family("Hmfma-trips")
    assert all(max(r["expect"]["trips"]) >= 2 and dg.h_on_matrix_cores(r) and r["n"] in (344, 352) for r in trips)
    got = {(r["k"], r["tile_px"]) for r in trips}
    assert got == {(13, 256), (16, 256), (13, 128), (16, 128), (24, 128)}
    for kt in got:   # both variants: rows of X off 16 bytes (u8, n_pad = 344) and on them
        mine = [r for r in trips if (r["k"], r["tile_px"]) == kt]
        assert any(r["expect"]["guarded"] for r in mine) and any(not r["expect"]["guarded"] for r in mine), kt
    assert {r["store"] for r in trips} == set(dg.STORES)
    gpb = _by_family("Wmfma-gpb")
    assert {(r["k"], r["store"]) for r in gpb} == {(k, s) for k in (9, 16, 24) for s in ("u8", "f32")}
    for r in gpb:
        blocks = r["expect"]["blocks"]
        assert r["expect"]["gpb"] == 3 and any(b[1] >= 1 for b in blocks) and any(b[2] for b in blocks) and any(b[3] for b in blocks)


def test_x_tile_rows():
    rows = _by_family("XTILE")
    for geo in ((128, 256), (128, 512), (256, 512)):
        for store in dg.STORES:
            mine = [r for r in rows if (r["tile_px"], r["x_tile"]) == geo and r["store"] == store]
            assert any(dg.h_on_matrix_cores(r) for r in mine) and any(not dg.h_on_matrix_cores(r) for r in mine), (geo, store)
    assert all(r["shape"] == (19, 37) and r["w_step"] and r["fit"] for r in rows)
    assert any(dg.w_on_matrix_cores(r) for r in rows)      # (w_accum_mfma_kernel addresses x_cm through x_tile too)


def test_which_rows_run_the_three_iterations():
    for fam in ("XTILE", "Wring", "Wmfma-gpb", "Hmfma-trips", "H128-ring"):
        assert all(r["fit"] for r in _by_family(fam)), fam
    for fam in ("XTILE", "Wring", "Wmfma-gpb"):
        assert all(r["w_step"] for r in _by_family(fam)), fam
