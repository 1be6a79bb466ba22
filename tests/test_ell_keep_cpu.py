"""The policy of the kept part of streamed lists (espm_amd/ell.py: keep_indices, keep_group_bytes, keep_policy; include/espm_mu.h:
ell_keep_h, ell_keep_w) - pure functions, no GPU."""
import os

import numpy as np
import pytest
import torch

from espm_amd import _lib, ell

MB = 10 ** 6
# the headline image's shape of things: 8 list groups per tile by decreasing length (230 MB), 32 channel groups (234 MB)
BYTES_H = [int(v) for v in np.linspace(40, 17.5, 8) * MB]
BYTES_W = [int(v) for v in np.linspace(12, 2.6, 32) * MB]


def _kept(sizes, keep):
    return sum(sizes[j] for j in ell.keep_indices(keep, len(sizes)))


@pytest.mark.parametrize("n", [1, 3, 8, 32, 33])
def test_kept_indices_are_spread_evenly(n):
    """keep of n: exactly `keep` indices, and every window of consecutive indices holds its share of them to within one - kept and
    streamed units alternate in the order they are handed out, never 'the first g groups'."""
    for keep in range(n + 1):
        idx = ell.keep_indices(keep, n)
        assert len(idx) == keep and idx == sorted(set(idx)) and all(0 <= j < n for j in idx)
        mark = np.zeros(n + 1, dtype=np.int64)
        mark[1:][idx] = 1
        cum = np.cumsum(mark)
        for a in range(n):
            for b in range(a + 1, n + 1):
                assert abs((cum[b] - cum[a]) - (b - a) * keep / n) < 1.0 + 1e-9, (keep, n, a, b)
    assert ell.keep_indices(0, n) == [] and ell.keep_indices(n, n) == list(range(n))


def test_the_rule_is_the_kernels():
    """floor((j + 1) keep / n) steps: the expression of ell_kept (csrc/mu_ell_kernel.hpp), spelled out for 4 of 8 and 3 of 8."""
    assert ell.keep_indices(4, 8) == [1, 3, 5, 7]
    assert ell.keep_indices(3, 8) == [2, 5, 7]
    assert ell.keep_indices(2, 3) == [1, 2]
    with open(os.path.join(os.path.dirname(ell.__file__), "csrc", "mu_ell_kernel.hpp")) as f:
        assert "return ((j + 1) * g) / n != (j * g) / n;" in f.read()


def test_kept_bytes_stay_within_the_budget_and_grow_with_it():
    last = (0, 0)
    for budget in range(0, 500 * MB, 3 * MB):
        stream, kh, kw = ell.keep_policy(BYTES_H, BYTES_W, budget)
        assert stream == 1 and 0 <= kh <= len(BYTES_H) and 0 <= kw <= len(BYTES_W)
        assert _kept(BYTES_H, kh) + _kept(BYTES_W, kw) <= budget
        assert kh >= last[0] and kw >= last[1], (budget, last, kh, kw)
        last = (kh, kw)
    assert last == (len(BYTES_H), len(BYTES_W))   # a budget beyond the lists keeps them all


def test_the_h_walk_is_kept_first_and_whole_before_the_w_walk():
    for budget in range(0, 500 * MB, 3 * MB):
        _, kh, kw = ell.keep_policy(BYTES_H, BYTES_W, budget)
        assert kw == 0 or kh == len(BYTES_H)
    # the headline at the header's budget: most of the H walk, nothing of the W walk
    _, kh, kw = ell.keep_policy(BYTES_H, BYTES_W, _lib.ELL_KEEP_BYTES)
    assert kw == 0 and 0.8 * _lib.ELL_KEEP_BYTES <= _kept(BYTES_H, kh) <= _lib.ELL_KEEP_BYTES


def test_nothing_is_kept_at_budget_zero():
    assert ell.keep_policy(BYTES_H, BYTES_W, 0) == (1, 0, 0)
    assert ell.keep_policy(BYTES_H, BYTES_W, -5) == (1, 0, 0)
    assert ell.keep_policy(BYTES_H, BYTES_W, min(BYTES_H) - 1) == (1, 0, 0)


def test_lists_that_fit_keep_todays_flags():
    """At or below ESPM_ELL_STREAM_BYTES: ell_stream = 0 and no keep values, whatever the budget."""
    small_h, small_w = [b // 4 for b in BYTES_H], [b // 4 for b in BYTES_W]
    assert sum(small_h) + sum(small_w) <= _lib.ELL_STREAM_BYTES < sum(BYTES_H) + sum(BYTES_W)
    for budget in (0, _lib.ELL_KEEP_BYTES, 10 ** 12):
        assert ell.keep_policy(small_h, small_w, budget) == (0, 0, 0)
    assert ell.keep_policy(BYTES_H, BYTES_W, _lib.ELL_KEEP_BYTES, list_bytes=_lib.ELL_STREAM_BYTES) == (0, 0, 0)
    assert ell.keep_policy(BYTES_H, BYTES_W, _lib.ELL_KEEP_BYTES, list_bytes=_lib.ELL_STREAM_BYTES + 1)[0] == 1
    assert ell.keep_policy(small_h, small_w, 10 ** 12, stream_bytes=0) == (1, len(small_h), len(small_w))   # (the A/B threshold of the engine)


def test_group_bytes_from_the_offset_arrays():
    """Rows of 256 bytes per (tile, list group) and per (block, channel group), summed by the group's index inside its tile / block."""
    rng = np.random.default_rng(5)
    gpt, tiles, n_cg, blocks = 8, 6, 5, 3
    rows_h = rng.integers(0, 50, size=tiles * gpt)
    rows_w = rng.integers(0, 70, size=blocks * n_cg)

    def offsets(rows):   # two words per group: first row, first general row; one closing word
        beg = np.concatenate([[0], np.cumsum(rows)])
        off = np.empty(2 * len(rows) + 1, dtype=np.int32)
        off[0::2] = beg
        off[1::2] = beg[:-1] + rows // 2
        return torch.from_numpy(off)
    bh, bw = ell.keep_group_bytes(offsets(rows_h), offsets(rows_w), gpt, n_cg)
    assert bh == [int(v) for v in rows_h.reshape(tiles, gpt).sum(0) * 256]
    assert bw == [int(v) for v in rows_w.reshape(blocks, n_cg).sum(0) * 256]
