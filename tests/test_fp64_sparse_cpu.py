"""The sparse count store of the fp64 mode (include/espm_mu.h, "fp64 mode, sparse store") built by espm_amd.sparse64: both orders
decode back to X, the empty-line records are right, and the store selection keeps what does not qualify on the dense stores.

CPU only: the builder is torch tensor plumbing and runs on host tensors; the kernels that walk the store are exercised by
tests/test_gpu_fp64_sparse.py."""
import numpy as np
import pytest
import torch

from espm_amd import conf, sparse64

WB = sparse64.WBLOCK


def decode_h(store):
    n, p = store["n"], store["p"]
    elem = store["h_elem"].numpy().view(np.uint32)
    off = store["h_off"].numpy()
    X = np.zeros((n, p), dtype=np.int64)
    count = 0
    for g in range((p + 63) // 64):
        rows = (off[g + 1] - off[g]) // 64
        blockd = elem[off[g]:off[g + 1]].reshape(rows, 64)
        for lane in range(64):
            lst = blockd[:, lane]
            live = lst[lst != 0]
            assert np.array_equal(lst[:len(live)], live), "padding only behind a list"
            if len(live) == 0:
                continue
            q = 64 * g + lane
            assert q < p
            c = (live & 0xffff).astype(np.int64)
            assert np.all(np.diff(c) > 0), "channels ascending"
            X[c, q] = live >> 16
            count += len(live)
        if rows:
            assert (blockd[-1] != 0).any(), "a group is as long as its longest list"
    return X, count


def decode_w(store):
    n, p = store["n"], store["p"]
    elem = store["w_elem"].numpy().view(np.uint32)
    off = store["w_off"].numpy()
    nblk = (p + WB - 1) // WB
    assert store["nblk_w"] == nblk and len(off) == nblk * n + 1 and off[0] == 0
    X = np.zeros((n, p), dtype=np.int64)
    for b in range(nblk):
        for c in range(n):
            lst = elem[off[b * n + c]:off[b * n + c + 1]]
            qo = (lst & 0xffff).astype(np.int64)
            assert np.all(np.diff(qo) > 0), "pixels ascending"
            assert np.all(lst >> 16 > 0)
            X[c, b * WB + qo] = lst >> 16
    return X, int(off[-1])


def multiset(store):
    """(pixel, channel, count) of every element of each order, sorted."""
    n, p = store["n"], store["p"]
    Xh, Xw = decode_h(store)[0], decode_w(store)[0]
    return [np.stack(np.nonzero(X.T) + (X.T[np.nonzero(X.T)],)) for X in (Xh, Xw)]


@pytest.mark.parametrize("n,p,layout,dtype", [(100, 333, "cm", np.float64), (70, WB + 77, "pm", np.int32), (130, 2 * WB + 5, "cm", np.float32),
                                               (64, 128, "pm", np.uint8)])
def test_both_orders_decode_to_x(n, p, layout, dtype):
    rng = np.random.default_rng(n + p)
    X = rng.poisson(0.15 * rng.uniform(0.2, 2.0, size=(n, 1)), size=(n, p)).astype(np.int64)
    empty_c, empty_p = [3, n // 2, n - 1], [0, p // 3, p - 1]
    if dtype != np.uint8:   # counts at the top of the range (the dword's sign bit set)
        X[rng.integers(0, n, 25), rng.integers(0, p, 25)] = 65535
        X[rng.integers(0, n, 25), rng.integers(0, p, 25)] = rng.integers(256, 65535, 25)
    X[empty_c, :] = 0
    X[:, empty_p] = 0
    given = np.ascontiguousarray((X if layout == "cm" else X.T).astype(dtype))
    use, note, stats = sparse64.select(given, layout, "auto")
    assert use and note == "" and stats["complete"]
    assert (stats["n"], stats["p"], stats["nnz"]) == (n, p, int((X != 0).sum()))
    store = sparse64.build(stats, fix_zero_lines=True)
    Xh, nh = decode_h(store)
    Xw, nw = decode_w(store)
    assert np.array_equal(Xh, X) and np.array_equal(Xw, X)
    assert nh == nw == store["nnz"] == int((X != 0).sum())
    mh, mw = multiset(store)
    assert np.array_equal(mh, mw)
    # the empty lines: recorded, not stored
    ec, ep = np.nonzero(X.sum(axis=1) == 0)[0], np.nonzero(X.sum(axis=0) == 0)[0]   # (the three set above, and what chance left empty)
    assert set(empty_c) <= set(ec.tolist()) and set(empty_p) <= set(ep.tolist())
    assert store["ec"].tolist() == ec.tolist() and store["n_ec"] == len(ec)
    assert store["ep"].tolist() == ep.tolist() and store["n_ep"] == len(ep)
    assert np.array_equal(store["ec_flag"].numpy().astype(bool), X.sum(axis=1) == 0)
    assert np.array_equal(store["ep_flag"].numpy().astype(bool), X.sum(axis=0) == 0)
    nblk = (p + WB - 1) // WB
    assert store["ep_off"].tolist() == [int((ep < b * WB).sum()) for b in range(nblk + 1)]
    assert int(store["hist"].sum()) == store["nnz"] and int(store["hist"][65535]) == int((X == 65535).sum())
    # const_KL and sum(X) of the filled image, against the dense formula (base.py:200-201)
    eps, xscale = 1e-14, 0.37
    Xf = X.astype(np.float64)
    Xf[X.sum(axis=1) == 0, :] = eps
    Xf[:, X.sum(axis=0) == 0] = eps
    Xf *= xscale
    c_kl, sum_x = sparse64.constants(store, xscale, eps)
    ref = float((Xf * np.log(np.maximum(Xf, eps)) - Xf).sum())
    assert abs(c_kl - ref) <= 1e-12 * abs(ref) and abs(sum_x - Xf.sum()) <= 1e-12 * Xf.sum()


def test_without_the_fill_no_line_is_recorded():
    X = np.zeros((40, 70), dtype=np.int64)
    X[5, 6] = 2
    store = sparse64.build(sparse64.select(X, "cm", "sparse")[2], fix_zero_lines=False)
    assert store["ec"] is None and store["ep"] is None and store["ep_off"] is None and store["n_ec"] == store["n_ep"] == 0
    assert np.array_equal(decode_h(store)[0], X) and np.array_equal(decode_w(store)[0], X)


def test_lines_the_caller_filled_count_as_empty():
    """The estimator hands over X with its empty lines already at log_shift and their masks (espm/estimators/base.py:519-528)."""
    rng = np.random.default_rng(4)
    X = rng.poisson(0.2, size=(50, 90)).astype(np.float64)
    X[:, 0] += 1
    X[0, :] += 1
    fc, fp = np.zeros(50, bool), np.zeros(90, bool)
    fc[[7, 20]] = True
    fp[33] = True
    X[fc, :] = 1e-14
    X[:, fp] = 1e-14
    use, note, stats = sparse64.select(X.T.copy(), "pm", "auto", filled_channels=fc, filled_pixels=fp)
    assert use, note
    store = sparse64.build(stats, fix_zero_lines=False)
    Xz = X.copy()
    Xz[fc, :] = 0
    Xz[:, fp] = 0
    assert np.array_equal(decode_h(store)[0], Xz) and np.array_equal(decode_w(store)[0], Xz)
    assert store["ec"].tolist() == [7, 20] and store["ep"].tolist() == [33]
    assert not sparse64.select(X, "cm", "auto")[0]   # (without the masks the fill makes it a float image)


def sparse_counts(rng, n=60, p=200):
    return rng.poisson(0.1, size=(n, p)).astype(np.float64)


@pytest.mark.parametrize("spoil,word", [("float", "integer counts"), ("negative", "negative"), ("large", "65536"), ("dense", "non-zero")])
def test_what_does_not_qualify_stays_dense(spoil, word):
    rng = np.random.default_rng(1)
    X = sparse_counts(rng)
    assert sparse64.select(X, "cm", "auto")[:2] == (True, "")
    assert sparse64.select(X, "cm", "sparse")[0]
    if spoil == "float":
        X[3, 4] = 0.5
    elif spoil == "negative":
        X[3, 4] = -1.0
    elif spoil == "large":
        X[3, 4] = 65536.0
    else:
        X = rng.poisson(-np.log(1 - min(0.95, conf.fp64_sparse_max_density + 0.1)), size=X.shape).astype(np.float64)
    use, note, stats = sparse64.select(X, "cm", "auto")
    assert not use and note.startswith("dense store") and word in note and stats["keys"] is None
    if spoil == "dense":   # density is the engineer's choice, not a property of the store: forcing it is allowed
        assert sparse64.select(X, "cm", "sparse")[0]
    else:
        with pytest.raises(ValueError, match="does not fit the sparse store"):
            sparse64.select(X, "cm", "sparse")


def test_threshold_keeps_half_full_images_dense():
    """tests/test_gpu_fp64.py pins the dense stores for Poisson images with 0.6 and more of their entries non-zero."""
    assert 0 < conf.fp64_sparse_max_density < 0.5
