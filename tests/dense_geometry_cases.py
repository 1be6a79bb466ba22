"""The table of tests/test_gpu_dense_geometry.py: the dense stores (u8, bf16, f32) at the tile and block sizes that large images get
("geometry of the dense stores"), on images of a few hundred pixels.  tests/test_dense_geometry_cpu.py holds the
`expect` column to the loops' own arithmetic without a GPU; the GPU test asserts the geometry on the engine's state and runs the row
against the fp64 oracle.  No torch, no GPU at import.

A row: id, family, k, store, tile_px, x_tile (None: tile_px), n, shape (nx, ny), m (None: G = identity), w_blocks (None: what
espm_mu_query gives, ceil(p / 16) blocks of 16 pixels at these sizes), fused (False: the vector kernels where the matrix cores would
run), rule ("kl": the default H rule; "l2": the Frobenius branch; "hq": h_rule 1; "pg": h_rule 2), opt (simplex_H / simplex_W,
lambda_L, mu), w_step / fit (whether the GPU test also runs one W step / three iterations), and `expect`: what the row is there for
(`why`) and the loop shapes it must produce, written out by hand - the CPU test recomputes them.

The loops.  The H step's channel loop (mu_h_kernel.hpp:688-739) and the W accumulation's pixel loop (mu_w_kernel.hpp:80-128) share one
shape: `count` items in groups of `unit`, a register ring of NBUF load groups whose steady-state loop takes 2 NBUF groups per trip,
a drain of the up to NBUF groups still in the ring, a plain loop over the remaining full groups and single items behind it
(`ring_shape`).  Which instance runs (mu_h_step.hip, mu_w_accum.hip):
  H, tile 256: NW = 4 waves, U = 8, NBUF = 0            H, tile 128: NW = 8, U = 8, NBUF = 2        (every store)
  W, u8: UP = 4, NBUF = 3                                W, bf16 / f32: UP = 4, NBUF = 0
  matrix cores: the H step from 13 components on (its channel loop: tiles of 64 channels dealt to 4 waves, mu_h_mfma_kernel.hpp:113),
  the W accumulation from 9 on (groups of 64 pixels, gpb per block, the next group's H' requested ahead, mu_w_mfma_kernel.hpp:216-230);
  fused=False keeps the vector kernels - which the 17..32 build has for the fp32 store only."""

STORES = ("u8", "bf16", "f32")
H_LOOP = {256: (4, 8, 0), 128: (8, 8, 2)}                 # tile_px -> (NW, U, NBUF) of h_step_kernel
W_LOOP = {"u8": (4, 3), "bf16": (4, 0), "f32": (4, 0)}    # store -> (UP, NBUF) of w_accum_kernel
H_MFMA_MIN_K, W_MFMA_MIN_K = 13, 9


def ring_shape(count, unit, nbuf):
    """(trips, drained, plain_groups, singles) of the loop that mu_h_kernel.hpp:688-739 (channels of a wave, unit U) and
    mu_w_kernel.hpp:80-128 (pixels of a block, unit UP) share: trips of the steady-state loop `for (; g + 2 * NBUF <= ngroups; g += 2 *
    NBUF)`, groups taken out of the ring behind it (at most NBUF), full groups left to the plain loop, items taken one at a time.
    NBUF < 2: no ring, every full group is a plain one."""
    ngroups, singles = count // unit, count % unit
    if nbuf < 2:
        return 0, 0, ngroups, singles
    trips = ngroups // (2 * nbuf)
    left = ngroups - trips * 2 * nbuf
    drained = min(nbuf, left)
    return trips, drained, left - drained, singles


def h_wave_shapes(n, tile_px):
    """ring_shape of every wave of an H tile: the waves split the n channels in chunks of ceil(n / NW), the last one shorter."""
    nw, unit, nbuf = H_LOOP[tile_px]
    chunk = -(-n // nw)
    out = []
    for wave in range(nw):
        begin = min(n, wave * chunk)
        out.append(ring_shape(min(n, begin + chunk) - begin, unit, nbuf))
    return out


def w_geometry(p, w_blocks):
    """(ppb, nblk_w) as MUEngine(w_blocks=) and espm_mu_query set them: whole pixels per block, then the blocks that leaves."""
    ppb = -(-p // w_blocks)
    return ppb, -(-p // ppb)


def default_w_blocks(p):
    """What espm_mu_query gives an image below 8192 pixels (2 CUs' worth of blocks is more than ceil(p / 16)): blocks of 16 pixels."""
    return -(-p // 16)


def w_block_shapes(p, w_blocks, store):
    """ring_shape of every pixel block of the vector W accumulation, the last block shorter."""
    unit, nbuf = W_LOOP[store]
    ppb, nblk = w_geometry(p, w_blocks)
    return [ring_shape(min(p, (b + 1) * ppb) - b * ppb, unit, nbuf) for b in range(nblk)]


def n_pad_of(n):
    return -(-n // 8) * 8


def mfma_h_trips(n):
    """Trips of `for (T = wave; T < tiles; T += 4)` per wave of the matrix-core H step: tiles of 64 channels of n_pad."""
    tiles = -(-n_pad_of(n) // 64)
    return [len(range(wave, tiles, 4)) for wave in range(4)]


def mfma_h_guarded_rows(n, store):
    """Whether the rows of the pixel-major X start off 16 bytes, so that every load of the matrix-core H step takes the guarded path
    (mu_h_mfma_kernel.hpp:48): one-byte elements with n_pad no multiple of 16."""
    return store == "u8" and n_pad_of(n) % 16 != 0


def mfma_w_groups(p, nblk_w):
    """Per block of the matrix-core W accumulation: (groups of 64 pixels worked, H' prefetches issued, a partial group among them, left
    by the `px0 >= p` exit) - gpb = ceil(p_pad / 64 / nblk_w) groups per block."""
    groups = -(-p // 512) * 512 // 64
    gpb = -(-groups // nblk_w)
    out = []
    for b in range(nblk_w):
        g0, g1 = b * gpb, min(groups, (b + 1) * gpb)
        worked = [g for g in range(g0, g1) if g * 64 < p]
        exits = len(worked) < g1 - g0
        prefetch = sum(1 for g in worked if g + 1 < g1)
        out.append((len(worked), prefetch, any(g * 64 + 64 > p for g in worked), exits))
    return gpb, out


def x_tile_terms(p, tile_px, x_tile):
    """Of the H tiles of an image: how many have tile0 / x_tile >= 1, how many tile0 % x_tile != 0 - the two terms of the X address
    (tile0 / x_tile) * n_cm * x_tile + tile0 % x_tile."""
    tiles = range(0, p, tile_px)
    return sum(1 for t in tiles if t // x_tile >= 1), sum(1 for t in tiles if t % x_tile != 0)


def build_of(k):
    """The component stride of the build that holds k components."""
    return 8 if k <= 8 else 16 if k <= 16 else 32


def h_on_matrix_cores(row):
    return row["fused"] and row["k"] >= H_MFMA_MIN_K and row["rule"] == "kl"


def w_on_matrix_cores(row):
    return row["fused"] and row["k"] >= W_MFMA_MIN_K


def matrix_core_row(row):
    """The rows held to their vector twin (fused=False) as well: the H step on the matrix cores, or the family that is there for the
    matrix-core W accumulation."""
    return h_on_matrix_cores(row) or row["family"] == "Wmfma-gpb"


# ---- options: the three the H256 rows alternate over, each on every store -----------------------------------------------------------
SH = dict(simplex_H=True, simplex_W=False, lambda_L=0.3, mu=0.05)     # simplex over H with the Laplacian and mu
SW = dict(simplex_H=False, simplex_W=True, lambda_L=0.0, mu=0)        # simplex over W
NO = dict(simplex_H=False, simplex_W=False, lambda_L=0.5, mu=0)       # neither
SH0 = dict(simplex_H=True, simplex_W=False, lambda_L=0.0, mu=0.02)
# The matrix-core rows all keep H on the simplex: their bound against the vector twin, max |dH| < 2e-5, is absolute - the project's
# figure for an H whose columns sum to 1 (tests/test_gpu_fullsize.py) - and means nothing for an H that carries the counts' scale.
RULE_OPT = dict(l2=dict(simplex_H=False, simplex_W=False, lambda_L=0.0, mu=0),      # (updates.py:109-118 has neither term)
                hq=dict(simplex_H=False, simplex_W=False, lambda_L=0.3, mu=0),
                pg=dict(simplex_H=False, simplex_W=False, lambda_L=0.3, mu=0.05))
# (without the simplex: the oracle restates the reference's bisection for these rules, converged to 1e-5 only, and the one-step
#  tolerance with the simplex, 3e-5, is the exact root's)

IMG = (19, 23)       # 437 pixels: p_pad 512; tile 256: a full tile and one of 181 pixels; tile 128: three full tiles and one of 53
IMG24 = (19, 24)     # 456 pixels = 19 blocks of exactly 24
IMGX = (19, 37)      # 703 pixels: p_pad 1024, two pixel blocks of x_tile = 512

H256_SHAPES = [(0, 0, 4, 4), (0, 0, 4, 6)]            # n = 150 over 4 waves: 38, 38, 38, 36 channels
H128_N150_SHAPES = [(0, 2, 0, 1), (0, 2, 0, 3)]       # n = 150 over 8 waves: 7 x 19 and 17 channels - the drain alone
RING_N = {256: ("one trip and nothing after", [(1, 0, 0, 0)]),                               # 8 x 32 channels
          344: ("one trip, a partial drain and singles", [(1, 1, 0, 3)]),                     # 8 x 43
          500: ("one trip, a full drain, a plain group and singles", [(1, 2, 1, 3), (1, 2, 1, 7)]),   # 7 x 63 and 59
          520: ("two trips", [(2, 0, 0, 1)])}                                                 # 8 x 65
# w_blocks on the 437 pixels -> (ppb, nblk_w, the blocks' shapes with NBUF = 3, what they are there for).  ceil(437 / w_blocks) never
# is 24 (w_blocks 18 gives 25, 19 gives 23): the block of exactly six groups is on 19 x 24 pixels, IMG24, with w_blocks = 19.
WRING = {18: (25, 18, [(0, 3, 0, 0), (1, 0, 0, 1)], "one trip, nothing drained, a single; the last block (12 pixels) the drain alone"),
         10: (44, 10, [(1, 3, 1, 1), (1, 3, 2, 0)], "one trip, a full drain, plain groups; the last block (41) with a single behind them"),
         9: (49, 9, [(1, 3, 2, 1), (2, 0, 0, 1)], "two trips; the last block (45) one trip, a full drain, plain groups and a single"),
         8: (55, 8, [(2, 1, 0, 0), (2, 1, 0, 3)], "two trips and a partial drain, with and (last block, 52) without singles")}
WRING24 = (24, 19, [(1, 0, 0, 0)], "exactly six groups: one trip and nothing after")
WPLAIN = (37, 12, [(0, 0, 7, 2), (0, 0, 9, 1)], "NBUF = 0: plain groups and singles (37 pixels, the last block 30)")

CASES = []


def _row(id, family, k, store, tile_px, n, opt, expect, *, x_tile=None, shape=IMG, m=None, w_blocks=None, fused=True, rule="kl",
         w_step=False, fit=False):
    CASES.append(dict(id=id, family=family, k=k, store=store, tile_px=tile_px, x_tile=x_tile, n=n, shape=shape, m=m, w_blocks=w_blocks,
                      fused=fused, rule=rule, opt=dict(opt), w_step=w_step, fit=fit, expect=expect))


# ---- H256: every component count on every store at 256-pixel tiles (h_step_kernel<K, XT, 4, 4, ., 8, 0>, h_step_mfma_kernel<K, XT, ., 256>) -----
for si, store in enumerate(STORES):
    for k in range(1, 17):
        _row(f"h256-{store}-k{k}", "H256", k, store, 256, 150, (SH, SW, NO)[(k + si) % 3],
             dict(why="the 256-pixel vector instance of this component count and store", loop="h", shapes=H256_SHAPES),
             fused=k < H_MFMA_MIN_K, m=k + 5 if k in (4, 10) else None, w_step=k == 8, fit=k in (1, 5, 8, 9, 13, 16))
    for k in range(13, 17):
        _row(f"h256-{store}-k{k}-mfma", "H256", k, store, 256, 150, SH if k % 2 else SH0,
             dict(why="the 256-pixel matrix-core instance of this component count and store", loop="h_mfma", trips=[1, 1, 1, 0],
                  guarded=store == "u8"),   # (n_pad = 152: three channel tiles; one-byte rows off 16 bytes)
             fit=k in (13, 16))

# ---- H256-rules: the alternate rules' 256-pixel instances (launch_h_l2 / launch_h_rule<K, 4, 4, 8, 0, RULE>), fp32 store -------------------
for rule in ("l2", "hq", "pg"):
    for k in (1, 5, 8, 9, 16):
        _row(f"h256-{rule}-k{k}", "H256-rules", k, "f32", 256, 150, RULE_OPT[rule],
             dict(why=f"the 256-pixel instance of the {rule} H step", loop="h", shapes=H256_SHAPES), rule=rule, fused=k < H_MFMA_MIN_K)

# ---- H128-ring: the register ring of the 128-pixel vector instances (NW = 8, U = 8, NBUF = 2) ------------------------------------------------
for store in STORES:
    for k in (3, 8, 12):
        for n, (why, shapes) in RING_N.items():
            _row(f"h128-{store}-k{k}-n{n}", "H128-ring", k, store, 128, n, (SH, SW, NO)[(k + n // 8) % 3], dict(why=why, loop="h", shapes=shapes), fit=True)
for n, (why, shapes) in RING_N.items():   # the widest build's vector kernels (fp32 store only)
    _row(f"h128-f32-k20-n{n}", "H128-ring", 20, "f32", 128, n, SH if n % 16 else NO, dict(why=why + ", widest build", loop="h", shapes=shapes), fused=False, fit=True)

# ---- Hmfma-trips: more than four 64-channel tiles, so that waves take a second trip (mu_h_mfma_kernel.hpp:113) ----------------------------------
for k, tile, variants in ((13, 256, (("u8", 344), ("u8", 352), ("bf16", 344), ("f32", 352))),
                          (16, 256, (("u8", 344), ("bf16", 352), ("f32", 344))),
                          (13, 128, (("u8", 344), ("f32", 352))),
                          (16, 128, (("u8", 344), ("bf16", 352))),
                          (24, 128, (("u8", 344), ("u8", 352), ("bf16", 352), ("f32", 344)))):
    for store, n in variants:
        _row(f"hmfma-{store}-k{k}-t{tile}-n{n}", "Hmfma-trips", k, store, tile, n, SH if n == 344 else SH0,
             dict(why="six channel tiles: two waves take a second trip" + ("; rows of X off 16 bytes: the guarded load" if store == "u8" and n == 344 else ""),
                  loop="h_mfma", trips=[2, 2, 1, 1], guarded=store == "u8" and n == 344), fit=True)

# ---- XTILE: x_tile != tile_px, both terms of the X address (H kernels, w_accum_mfma_kernel) ------------------------------------------------------
for tile, xt, terms, vec_k, mf_k in ((128, 256, (4, 3), (5, 7, 11), (13, 24, 16)),
                                     (128, 512, (2, 4), (7, 11, 5), (24, 16, 13)),
                                     (256, 512, (1, 1), (11, 5, 7), (16, 13, 14))):
    for si, store in enumerate(STORES):
        for k, kind in ((vec_k[si], "vector"), (mf_k[si], "mfma")):
            loop = dict(loop="h", shapes=H256_SHAPES if tile == 256 else H128_N150_SHAPES) if kind == "vector" else dict(loop="h_mfma", trips=[1, 1, 1, 0], guarded=store == "u8")
            _row(f"xtile-{tile}-{xt}-{store}-k{k}", "XTILE", k, store, tile, 150, SH if kind == "mfma" else (SW, NO, SH)[si], x_tile=xt, shape=IMGX,
                 expect=dict(why=f"tiles {tile} in blocks of {xt}: {terms[0]} tiles with tile0 / x_tile >= 1, {terms[1]} with tile0 % x_tile != 0"
                             + ("; the matrix-core W accumulation reads x_cm too" if k >= W_MFMA_MIN_K else ""), x_terms=terms, **loop),
                 w_step=True, fit=True)

# ---- Wring: the register ring of the 8-bit store's vector W accumulation (w_accum_kernel<K, uint8_t, CH, 4, 3>) ------------------------------------
for k in (2, 5, 8, 12):   # (8 channels per lane up to 8 components, 4 beyond: fused=False keeps the vector kernel there)
    for wb in (18, 10, 9) + ((8,) if k == 5 else ()):
        ppb, nblk, shapes, why = WRING[wb]
        _row(f"wring-u8-k{k}-b{wb}", "Wring", k, "u8", 128, 150, (SW, NO, SH)[(k + wb) % 3], dict(why=why, loop="w", ppb=ppb, nblk_w=nblk, shapes=shapes),
             w_blocks=wb, fused=k <= 8, m=11 if (k, wb) == (5, 10) else None, w_step=True, fit=True)
for k in (5, 12):
    ppb, nblk, shapes, why = WRING24
    _row(f"wring-u8-k{k}-24", "Wring", k, "u8", 128, 150, SW, dict(why=why, loop="w", ppb=ppb, nblk_w=nblk, shapes=shapes), shape=IMG24, w_blocks=19,
         fused=k <= 8, w_step=True, fit=True)
for store in ("bf16", "f32"):
    ppb, nblk, shapes, why = WPLAIN
    _row(f"wring-{store}-k5-b12", "Wring", 5, store, 128, 150, NO if store == "bf16" else SW, dict(why=why, loop="w", ppb=ppb, nblk_w=nblk, shapes=shapes),
         w_blocks=12, w_step=True, fit=True)

# ---- Wmfma-gpb: three 64-pixel groups per block of the matrix-core W accumulation ------------------------------------------------------------------
for k in (9, 16, 24):
    for store in ("u8", "f32"):
        _row(f"wmfma-{store}-k{k}", "Wmfma-gpb", k, store, 128, 150, SH if store == "u8" else SH0,
             dict(why="gpb = 3: the H' prefetch runs, the last block holds the partial group 384..447 and leaves at group 448..", loop="w_mfma", ppb=146,
                  nblk_w=3, gpb=3, blocks=[(3, 2, False, False), (3, 2, False, False), (1, 1, True, True)]),
             w_blocks=3, w_step=True, fit=True)


# ---- what the rows, taken together, must show: (kernel family, NBUF) -> {class: predicate on a ring_shape} -------------------------------------------
REQUIRED_RING = {
    ("h", 2): {"one trip and nothing after": lambda s: s == (1, 0, 0, 0),
               "one trip, a partial drain and singles": lambda s: s[0] == 1 and 0 < s[1] < 2 and s[2] == 0 and s[3] > 0,
               "one trip, a full drain, a plain group and singles": lambda s: s[0] == 1 and s[1] == 2 and s[2] >= 1 and s[3] > 0,
               "two trips": lambda s: s[0] == 2},
    ("h", 0): {"plain groups and singles": lambda s: s[0] == 0 and s[1] == 0 and s[2] >= 1 and s[3] > 0},
    ("w", 3): {"exactly six groups": lambda s: s == (1, 0, 0, 0),
               "one trip, a full drain, plain groups and singles": lambda s: s[0] == 1 and s[1] == 3 and s[2] >= 1 and s[3] > 0,
               "two trips": lambda s: s[0] == 2},
    ("w", 0): {"plain groups and a single": lambda s: s[0] == 0 and s[1] == 0 and s[2] >= 1 and s[3] == 1},
}
