"""Constants of the multiplicative-update path (espm/conf.py:55-59)."""
log_shift = 1e-14
dicotomy_tol = 1e-5
seed_max = 4294967295
sigmaL = 8
maxit_dichotomy = 100
# fp64 mode: x_store="auto" takes the sparse count store (espm_amd/sparse64.py) up to this share of non-zero entries, from this many
# entries of X on.  Measured: the sparse path is 2.5x faster than the dense one at 0.4 at the headline size and
# 1.3x at 1980 x 128^2, the densest images timed, so the crossover lies above; 0.4 is claimed, and no lower size limit.
fp64_sparse_max_density = 0.4
fp64_sparse_min_entries = 0
