"""The sparse count store of the fp64 mode (include/espm_mu.h, "fp64 mode, sparse store"): which images take it, and its builder.

Plumbing only (torch tensor operations on the device that holds X, host tensors included): the store is built once per fit; the
kernels that walk it are in espm_amd/csrc/mu_fp64_sparse.hip.  X is read in row chunks in its own dtype: no fp64 copy of the image.

Layout (the header is the authoritative description): one dword per non-zero element, count << 16 | index, in two orders.
  H order  the lists of 64 consecutive pixels interleaved dword-wise, channels ascending, padded with 0 to the group's longest list
  W order  plain CSR by (block of F64S_WBLOCK pixels, channel), pixel offsets ascending
Lines without a count are not stored: ``ec`` / ``ep`` record them and the kernels apply the reference's log_shift fill.
"""
from __future__ import annotations

import math

import torch

from . import _lib, conf

MAX_COUNT, MAX_N, WBLOCK = _lib.F64S_MAX_COUNT, _lib.F64S_MAX_N, _lib.F64S_WBLOCK
_CHUNK = 16 << 20   # entries of X looked at per step


def _chunks(X, layout, filled_channels, filled_pixels, device):
    """Row chunks of X on ``device`` (X's own when None), the lines of the two masks (the caller filled them) set to 0."""
    rmask, cmask = (filled_channels, filled_pixels) if layout == "cm" else (filled_pixels, filled_channels)
    step = max(1, _CHUNK // max(1, X.shape[1]))
    for a in range(0, X.shape[0], step):
        xs = X[a:a + step]
        if device is not None:
            xs = xs.to(device)
        if rmask is not None or cmask is not None:
            xs = xs.clone()
            if rmask is not None:
                xs[rmask[a:a + step]] = 0
            if cmask is not None:
                xs[:, cmask] = 0
        yield a, xs


def scan(X, layout="cm", x_store="auto", filled_channels=None, filled_pixels=None, device=None, max_density=None):
    """One pass over the 2-D tensor X ((n, p) for layout 'cm', (p, n) for 'pm') in row chunks, each moved to ``device``: what the
    store selection needs to know (n, p, nnz, whether every entry is a non-negative integer, the largest entry, which channels /
    pixels hold a count) and, while the image still qualifies, its non-zero elements as int64 keys pixel << 32 | channel << 16 |
    count.  The pass ends at the first chunk that disqualifies the image (under "auto": also once more than max_density of ALL
    entries are known to be non-zero): ``complete`` tells whether it saw everything.  filled_channels / filled_pixels: boolean masks
    of lines the caller filled with log_shift (base.py:519-528); their entries count as zeros."""
    if X.dim() != 2 or layout not in ("cm", "pm"):
        raise ValueError("X must be 2-D and layout 'cm' or 'pm'")
    max_density = conf.fp64_sparse_max_density if max_density is None else max_density
    dev = X.device if device is None else torch.device(device)
    masks = [None if m is None else torch.as_tensor(m, dtype=torch.bool).to(dev) for m in (filled_channels, filled_pixels)]
    n, p = (X.shape[0], X.shape[1]) if layout == "cm" else (X.shape[1], X.shape[0])
    rows_any, cols_any = torch.zeros(X.shape[0], dtype=torch.bool, device=dev), torch.zeros(X.shape[1], dtype=torch.bool, device=dev)
    nnz, integral, negative, xmax, complete, keys = 0, X.dtype != torch.bool, False, 0.0, True, []
    limit = max_density * n * p if x_store == "auto" else float("inf")
    fits = n <= MAX_N and n * p > 0
    for a, xs in _chunks(X, layout, masks[0], masks[1], dev):
        nz = xs != 0
        nnz += int(nz.sum())
        rows_any[a:a + xs.shape[0]] = nz.any(dim=1)
        cols_any |= nz.any(dim=0)
        if xs.dtype.is_floating_point:   # (a NaN or an infinity is not a count)
            integral = integral and bool(((xs == torch.round(xs)) & torch.isfinite(xs)).all())
        if xs.dtype != torch.uint8:
            negative = negative or bool((xs < 0).any())
        if xs.numel():
            xmax = max(xmax, float(xs.max()))
        if not (fits and integral and not negative and xmax <= MAX_COUNT and nnz <= limit):
            complete, keys = a + xs.shape[0] >= X.shape[0], None
            break
        idx = nz.nonzero()
        v = xs[idx[:, 0], idx[:, 1]].to(torch.int64)
        r, c = idx[:, 0] + a, idx[:, 1]
        q, ch = (c, r) if layout == "cm" else (r, c)
        keys.append((q << 32) | (ch << 16) | v)
        del nz, idx, v, r, c, q, ch
    chan, pix = (rows_any, cols_any) if layout == "cm" else (cols_any, rows_any)
    return dict(n=int(n), p=int(p), nnz=nnz, integral=integral, negative=negative, xmax=xmax, chan_any=chan, pix_any=pix, complete=complete,
                keys=keys, filled_channels=masks[0], filled_pixels=masks[1], device=dev)


def choose(stats, x_store="auto", max_density=None):
    """(True, "") when the image of ``stats`` (scan) goes on the sparse store, (False, why not) when it stays dense under
    x_store="auto"; x_store="sparse" raises ValueError instead of staying dense."""
    max_density = conf.fp64_sparse_max_density if max_density is None else max_density
    entries = stats["n"] * stats["p"]
    why = ""
    if stats["negative"]:
        why = "negative entries"
    elif not stats["integral"]:
        why = "not an image of integer counts"
    elif stats["xmax"] > MAX_COUNT:
        why = f"a count of {stats['xmax']:.0f} (the store holds up to {MAX_COUNT})"
    elif stats["n"] > MAX_N:
        why = f"{stats['n']} channels (the store indexes up to {MAX_N})"
    elif entries == 0:
        why = "an empty image"
    elif x_store == "auto" and stats["nnz"] > max_density * entries:
        why = f"{'more than ' if not stats['complete'] else ''}{stats['nnz'] / entries:.3f} of the entries are non-zero (sparse up to {max_density})"
    elif x_store == "auto" and entries < conf.fp64_sparse_min_entries:
        why = f"{entries} entries (sparse from {conf.fp64_sparse_min_entries})"
    if why and x_store == "sparse":
        raise ValueError(f"fp64 mode: X does not fit the sparse store: {why}")
    return (not why), (f"dense store: {why}" if why else "")


def select(X, layout="cm", x_store="auto", **kw):
    """scan + choose for a tensor or array X: (use_sparse, note, stats).  Needs no GPU."""
    Xt = X if isinstance(X, torch.Tensor) else torch.as_tensor(X)
    stats = scan(Xt, layout, x_store, **kw)
    use, note = choose(stats, x_store)
    return use, note, stats


def _dwords(hi16, lo16):
    """int32 tensor of hi16 << 16 | lo16 (int64 inputs below 65536; the bit pattern of the unsigned dword)."""
    d = (hi16 << 16) | lo16
    return torch.where(d >= (1 << 31), d - (1 << 32), d).to(torch.int32)


def build(stats, fix_zero_lines=True):
    """The store of the image ``stats`` (scan) describes, which passed ``choose``, on the scan's device.  Returns a dict:
    n, p, nnz; h_elem (int32 dwords), h_off (int64); w_elem, w_off; ec, ec_flag, ep, ep_flag, ep_off (None without lines to fill:
    the masks the scan was given, else with fix_zero_lines the lines without a count); hist (int64, 65536): how many elements hold
    each count.  Consumes stats["keys"]."""
    n, p, dev = stats["n"], stats["p"], stats["device"]
    i64 = dict(dtype=torch.int64, device=dev)
    keys, stats["keys"] = stats["keys"], None
    kh = torch.sort(torch.cat(keys) if keys else torch.zeros(0, **i64))[0]   # by pixel, then channel (the keys are unique)
    del keys
    nnz = int(kh.numel())
    hist = torch.zeros(MAX_COUNT + 1, **i64)   # (by sorting: nearly every count is 1, which a histogram's atomics serialise)
    vals, cnts = torch.unique(kh & 0xffff, return_counts=True)
    hist[vals] = cnts
    del vals, cnts
    # ---- H order: groups of 64 pixels, interleaved
    ngrp = (p + 63) // 64
    q = kh >> 32
    lens = torch.bincount(q, minlength=ngrp * 64)
    h_off = torch.zeros(ngrp + 1, **i64)
    h_off[1:] = torch.cumsum(lens.view(ngrp, 64).amax(dim=1) * 64, 0)
    start = torch.cumsum(lens, 0) - lens
    dest = torch.arange(nnz, **i64) - start[q]
    dest *= 64
    dest += h_off[q >> 6]
    dest += q & 63
    del q, start, lens
    h_elem = torch.zeros(max(1, int(h_off[-1])), dtype=torch.int32, device=dev)
    h_elem[dest] = _dwords(kh & 0xffff, (kh >> 16) & 0xffff)
    del dest
    # ---- W order: CSR by (block of pixels, channel)
    nblk = (p + WBLOCK - 1) // WBLOCK
    q = kh >> 32
    kw = (((q // WBLOCK) * n + ((kh >> 16) & 0xffff)) << 32) | ((q % WBLOCK) << 16) | (kh & 0xffff)
    del kh, q
    kw = torch.sort(kw)[0]
    w_off = torch.zeros(nblk * n + 1, **i64)
    w_off[1:] = torch.cumsum(torch.bincount(kw >> 32, minlength=nblk * n), 0)
    w_elem = torch.zeros(max(1, nnz), dtype=torch.int32, device=dev)
    w_elem[:nnz] = _dwords(kw & 0xffff, (kw >> 16) & 0xffff)
    del kw
    store = dict(n=n, p=p, nnz=nnz, nblk_w=nblk, h_elem=h_elem, h_off=h_off, w_elem=w_elem, w_off=w_off, hist=hist,
                 ec=None, ec_flag=None, ep=None, ep_flag=None, ep_off=None, n_ec=0, n_ep=0)
    given = stats["filled_channels"] is not None or stats["filled_pixels"] is not None
    if given or fix_zero_lines:   # espm/estimators/base.py:519-528: the lines the reference fills with log_shift
        if given:
            ec_flag = stats["filled_channels"] if stats["filled_channels"] is not None else torch.zeros(n, dtype=torch.bool, device=dev)
            ep_flag = stats["filled_pixels"] if stats["filled_pixels"] is not None else torch.zeros(p, dtype=torch.bool, device=dev)
        else:
            ec_flag, ep_flag = ~stats["chan_any"], ~stats["pix_any"]
        ec, ep = ec_flag.nonzero()[:, 0], ep_flag.nonzero()[:, 0]
        if ec.numel():
            store.update(ec=ec.to(torch.int32), ec_flag=ec_flag.to(torch.uint8), n_ec=int(ec.numel()))
        if ep.numel():
            edges = torch.arange(nblk + 1, **i64) * WBLOCK
            store.update(ep=ep.to(torch.int32), ep_flag=ep_flag.to(torch.uint8), n_ep=int(ep.numel()),
                         ep_off=torch.searchsorted(ep, edges).to(torch.int32))
    return store


def constants(store, xscale, log_shift):
    """(const_KL, sum_x) of the effective image (base.py:200-201): sum(x log max(x, log_shift) - x) and sum(x) over the elements
    (through the histogram of their counts) plus the closed form of the filled entries, each log_shift * xscale."""
    cnt = store["hist"].to(torch.float64).cpu()
    xs = torch.arange(cnt.numel(), dtype=torch.float64) * xscale
    c_kl = float((cnt * (xs * torch.log(xs.clamp_min(log_shift)) - xs)).sum())
    sum_x = float((cnt * xs).sum())
    filled = store["n_ec"] * store["p"] + store["n_ep"] * store["n"] - store["n_ec"] * store["n_ep"]
    f = log_shift * xscale
    if filled:
        c_kl += filled * (f * math.log(max(f, log_shift)) - f)
        sum_x += filled * f
    return c_kl, sum_x
