"""The table of tests/test_gpu_w_update_forms.py: one row per form of the W update and per edge of its dispatch (DESIGN.md section 4,
"forms of the W update").  tests/test_w_update_form_cpu.py checks the `expect` column against the library's plan without a GPU; the
GPU test asserts it again on the engine's own state and then runs the row against the fp64 oracle.

No predicate of the dispatch depends on the pixel count, so every row fits a 6 x 7 image.

A row: (id, k, n, m, options, expected form, expected detail).  k picks the build (1..8, 9..16, 17..32).  m = None: G = identity.
Options: simplex_W; rows (simplex_W over a subset of the rows of W); fixed (fixed_W); algo "pg" (projected gradient, gamma drawn as
in tests/test_gpu_fuzz.py) or "bmd" (the Bregman variant); no_scratch (the workspace of the many-workgroup forms withheld, as in
test_local_w_update_equals_the_one_workgroup_finish: G = identity without the simplex then takes a one-workgroup finish); frac
(fractional data: the dense fp32 store).  Detail: (threads, rows per thread, channels per thread, all-threads G^T A) for the
register-resident finish, else None."""

LOCAL, SPLIT, COLUMNS, TWO, REGS, GENERAL = "local", "simplex_split", "dict_columns", "dict_two_launch", "one_wg_registers", "one_wg_general"


def _row(id, k, n, m, form, detail=None, **opt):
    return dict(id=id, k=k, n=n, m=m, form=form, detail=detail, opt=opt)


SW = dict(simplex_W=True)
ROWS = dict(simplex_W=True, rows=True)

CASES = [
    # ---- narrow build (k <= 8), dictionary, default rule -----------------------------------------------------------------------
    _row("n-dict-col-k1", 1, 200, 12, COLUMNS),
    _row("n-dict-col-second-channel-fixed", 5, 1030, 17, COLUMNS, fixed=True),          # a thread's second channel mostly absent
    _row("n-dict-col-limit", 8, 2048, 32, COLUMNS),                                     # m = 32 with n_pad = 2048
    _row("n-dict-two-9wg", 3, 2049, 32, TWO),                                           # n_pad 2056: 9 row workgroups, second trip of the update kernel
    _row("n-dict-two-5000", 5, 5000, 33, TWO),                                          # 20 row workgroups, two batches of G columns
    _row("n-dict-two-m70-fixed", 8, 300, 70, TWO, fixed=True),                          # three batches of G columns
    _row("n-dict-two-mk1040", 8, 300, 130, TWO),                                        # rel_W beyond the four preloaded entries per thread
    _row("n-dict-two-mk8192", 8, 300, 1024, TWO, frac=True),
    _row("n-dict-general-mk8200", 8, 300, 1025, GENERAL),
    _row("n-dict-general-5000", 3, 5000, 9, GENERAL),                                   # (2 m k 4 = 216 bytes of scratch < 1296)
    # ---- narrow build, dictionary in one workgroup ------------------------------------------------------------------------------
    _row("n-dict1-c1", 3, 150, 9, REGS, (1024, 1, 1, True), **SW),
    _row("n-dict1-c2", 3, 1500, 9, REGS, (1024, 1, 2, True), **SW),
    _row("n-dict1-c4", 3, 3000, 9, REGS, (1024, 1, 4, True), **SW),
    _row("n-dict1-c4-edge", 3, 4096, 9, REGS, (1024, 1, 4, True), **SW),
    _row("n-dict1-general-4097", 3, 4097, 9, GENERAL, **SW),
    _row("n-dict1-mk512", 8, 300, 64, REGS, (1024, 1, 1, True), **SW),
    _row("n-dict1-mk560", 8, 300, 70, REGS, (1024, 1, 1, False), **SW),
    _row("n-dict1-mk8192", 8, 300, 1024, REGS, (1024, 1, 1, False), **SW),              # m k = 8192 and exactly 64 KB of LDS
    _row("n-dict1-lds-edge", 5, 300, 1260, REGS, (1024, 2, 2, False), **SW),            # 65520 bytes of LDS
    _row("n-dict1-general-lds", 5, 300, 1261, GENERAL, **SW),                           # 65572
    _row("n-dict1-c2-rows", 3, 1500, 9, REGS, (1024, 1, 2, True), **ROWS),
    _row("n-dict1-c4-fixed", 3, 3000, 9, REGS, (1024, 1, 4, True), simplex_W=True, fixed=True),
    _row("n-dict1-c2-pg", 3, 1500, 9, REGS, (1024, 1, 2, True), algo="pg"),
    # (the simplex over every row of W divides a common factor of G^T A out again: a fourth channel's term scaled by 0.999 passed the
    #  rows above.  Rows of W outside the simplex, and the projected gradient, keep it - with a fourth channel that exists, n > 3072)
    _row("n-dict1-c4-edge-rows", 3, 4096, 9, REGS, (1024, 1, 4, True), **ROWS),
    _row("n-dict1-c4-edge-pg", 3, 4096, 9, REGS, (1024, 1, 4, True), algo="pg"),
    _row("n-dict1-c2-wave", 8, 1500, 70, REGS, (1024, 1, 2, False), **ROWS),            # (2 and 4 channels with the wave-per-entry G^T A:
    _row("n-dict1-c4-wave", 8, 3500, 70, REGS, (1024, 1, 4, False), **ROWS),            #  the completeness test asks for them)
    # ---- narrow build, G = identity ---------------------------------------------------------------------------------------------
    _row("n-id-local-64", 4, 64, None, LOCAL),
    _row("n-id-regs-63", 4, 63, None, REGS, (512, 1, 1, False)),
    _row("n-id-split-96", 4, 96, None, SPLIT, **SW),
    _row("n-id-regs-70", 4, 70, None, REGS, (512, 1, 1, False), **SW),                  # n_pad = 72 is no multiple of 32
    _row("n-id-rows-300", 5, 300, None, REGS, (512, 1, 1, False), **ROWS),
    _row("n-id-rows-1000", 5, 1000, None, REGS, (512, 2, 2, False), **ROWS),
    _row("n-id-rows-2048", 5, 2048, None, REGS, (512, 4, 4, False), **ROWS),
    _row("n-id-rows-2049", 5, 2049, None, REGS, (1024, 4, 4, False), **ROWS),
    _row("n-id-rows-4096", 5, 4096, None, REGS, (1024, 4, 4, False), **ROWS),
    _row("n-id-rows-4097", 5, 4097, None, GENERAL, **ROWS),
    # (the projected-gradient W step has no simplex over W - updates.py:368-369, the state check refuses it - so these rows reach the
    #  one-workgroup finish the way the Bregman rows do: the workspace withheld.  The general finish keeps its numerators in that
    #  workspace and refuses an update without it: with G = identity and no simplex it runs where n < 64 in the 17..32 build alone,
    #  the rows w32-id-pg-63 and w32-id-bmd-63 below.  The Bregman variant is built for n <= 4096, the state check refuses 4097.)
    _row("n-id-pg-1000", 5, 1000, None, REGS, (512, 2, 2, False), algo="pg", no_scratch=True),
    _row("n-id-bmd-1000", 5, 1000, None, REGS, (512, 2, 2, False), algo="bmd", no_scratch=True),
    _row("n-id-pg-4096", 5, 4096, None, REGS, (1024, 4, 4, False), algo="pg", no_scratch=True),
    _row("n-id-bmd-4096", 5, 4096, None, REGS, (1024, 4, 4, False), algo="bmd", no_scratch=True),
    # ---- wide build (k = 12): 1024 threads always, G^T A one wave per entry always ----------------------------------------------------
    _row("w-dict-col-limit", 12, 2048, 32, COLUMNS),
    _row("w-dict-two-2049", 12, 2049, 32, TWO),                                         # the scratch condition with KP = 16
    _row("w-dict1-c2", 12, 1500, 20, REGS, (1024, 1, 2, False), **SW),
    _row("w-dict1-general-4097", 12, 4097, 20, GENERAL, **SW),
    _row("w-id-rows-2048", 12, 2048, None, REGS, (1024, 2, 2, False), **ROWS),
    _row("w-id-local", 12, 150, None, LOCAL),                                           # (these five: what the completeness test asks of this build)
    _row("w-id-split", 12, 96, None, SPLIT, **SW),
    _row("w-dict1-c1", 12, 150, 20, REGS, (1024, 1, 1, False), **SW),
    _row("w-dict1-c4", 12, 3000, 20, REGS, (1024, 1, 4, False), **SW),
    _row("w-id-rows-4096", 12, 4096, None, REGS, (1024, 4, 4, False), **ROWS),
    # ---- widest build (k = 20, dense store): no register-resident finish ----------------------------------------------------------
    _row("w32-dict-two-3wg", 20, 600, 40, TWO),
    _row("w32-dict1-general", 20, 600, 40, GENERAL, **SW),
    _row("w32-id-local", 20, 150, None, LOCAL),
    _row("w32-id-split", 20, 96, None, SPLIT, **SW),
    _row("w32-dict-col", 20, 150, 30, COLUMNS, frac=True),
    _row("w32-id-pg-63", 20, 63, None, GENERAL, algo="pg"),
    _row("w32-id-bmd-63", 20, 63, None, GENERAL, algo="bmd"),
]

# the three column-form rows that the ESPM_W_GCOL=0 / ESPM_W_GSPLIT=0 children run
KNOB_CASES = [c for c in CASES if c["id"] in ("n-dict-col-k1", "n-dict-col-second-channel-fixed", "n-dict-col-limit")]


def build_of(k):
    """The component stride of the build that holds k components."""
    return 8 if k <= 8 else 16 if k <= 16 else 32


def reachable(kp):
    """Every (form, detail) the plan can return in the build of component stride kp, from the forms and the instances built
    (w_finish_fast_kernel<k, ROWS, NT, CROWS>: mu_w_finish.hip) - without the nt == 256 instances of the ESPM_WF_FEW_THREADS=256 A/B build.

    G = identity: ROWS = CROWS in {1, 2, 4}; 512 threads where k <= 8 and n_cm <= 2048 (so 1024 threads there begin at three rows per
    thread: ROWS 4), 1024 threads always in the 9..16 build.  Dictionary: 1024 threads; one row of W per thread with 1, 2 or 4
    channels, or ROWS = CROWS in {2, 4}; the all-threads G^T A needs m k <= 512 - one row per thread - and k <= 8."""
    out = {(f, None) for f in (LOCAL, SPLIT, COLUMNS, TWO, GENERAL)}
    if kp == 32:
        return out
    for c in (1, 2, 4):
        out.add((REGS, (1024, 1, c, False)))
        if kp == 8:
            out.add((REGS, (1024, 1, c, True)))
            out.add((REGS, (512, c, c, False)))
    out |= {(REGS, (1024, 2, 2, False)), (REGS, (1024, 4, 4, False))}
    return out
