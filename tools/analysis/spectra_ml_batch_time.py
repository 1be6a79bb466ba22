"""Time of espm_spectra_ml_pass_batch (csrc/mu_spectra_ml.hip) per model, and of espm_spectra_ml_pass after its body moved into a
device function that both kernels call, against the single pass of ANOTHER build of the library (the commit before the batch), and
of ``spectra_ml.intervals`` end to end, at the headline image (2048 channels x 512^2 pixels; bench.py's dose of 500 counts per pixel).

    python tools/analysis/spectra_ml_batch_time.py [--parent LIB] [--size n,nx,ny] [--k 5] [--x-dtype u8] [--batches 8,32] [--m 12]
                                                   [--runs 20] [--calls 10] [--out FILE]

1. The pass.  X is device-resident synthetic Poisson counts, drawn as 8-bit and held as --x-dtype (u8, u16, f32 or f64: the kernels are
   instantiated per element type).  For each layout the single pass of --parent (a libespm_mu.so
   built from the parent commit, opened beside this build's: only its espm_spectra_ml_pass is called; without --parent this build's
   own single pass is the yardstick), this build's single pass and the batch pass at every size of --batches are timed INTERLEAVED in
   one process: a window of each in turn, --runs times, HIP events around each window of about --calls single passes' work.
   Reported: the median and min - max per entry point, the ratio of the medians to the yardstick (the batch per model), the
   yardstick's own spread.  Model b of a batch is D (1 + b / 100); model 0's sums are compared bit for bit with both single passes.
2. End to end (--m > 0).  The dictionary of spectra_ml_time.py (the set-up in which ``presence`` is timed): ``intervals`` over all m k
   entries from W = 1 with the batch it chooses, and with batch=1 - wall time, passes, lockstep passes, the batch."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from espm_amd import _lib, spectra_ml  # noqa: E402
from espm_amd.conf import log_shift  # noqa: E402
from espm_amd.engine import _ptr, _stream, require_gpu  # noqa: E402

from pixel_diagnostics_time import CODES, COUNTS, draw, model  # noqa: E402  (the same image as the diagnostics)


def single(lib, X, layout, D, H, out, un, scratch):
    n, p = (X.shape[0], X.shape[1]) if layout == "cm" else (X.shape[1], X.shape[0])
    _lib.check(lib.espm_spectra_ml_pass(_ptr(X), CODES[X.dtype], _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM, int(X.stride(0)), n, p,
                                        _ptr(D), _ptr(H), D.shape[1], float(log_shift), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]),
                                        _ptr(out[4]), _ptr(un), _ptr(scratch), scratch.numel() * 8, _stream()), lib)


def batched(X, layout, Ds, H, out, un, scratch):
    n, p = (X.shape[0], X.shape[1]) if layout == "cm" else (X.shape[1], X.shape[0])
    _lib.check(_lib.lib.espm_spectra_ml_pass_batch(_ptr(X), CODES[X.dtype], _lib.LAYOUT_CM if layout == "cm" else _lib.LAYOUT_PM,
                                                   int(X.stride(0)), n, p, _ptr(Ds), _ptr(H), Ds.shape[2], Ds.shape[0], None, float(log_shift),
                                                   _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _ptr(un), _ptr(scratch),
                                                   scratch.numel() * 8, _stream()))


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def open_parent(path):
    """Another build of the library, for its single pass alone (its other symbols may differ from this header's)."""
    lib = ctypes.CDLL(path)
    for name in ("espm_spectra_ml_pass", "espm_mu_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--size", default="2048,512,512")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--x-dtype", default="u8", choices=["u8", "u16", "f32", "f64"])
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--m", type=int, default=12)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    require_gpu()
    n, nx, ny = (int(v) for v in args.size.split(","))
    p, k, m = nx * ny, args.k, args.m
    nt = k * (k + 1) // 2
    sizes = [int(v) for v in args.batches.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"spectra ML batch pass, {n} channels x {nx} x {ny} pixels, k = {k}, {args.x_dtype} X, 500 counts per pixel, {args.runs} interleaved windows, "
        f"{torch.cuda.get_device_name(0)}; yardstick: espm_spectra_ml_pass of {'the parent build' if args.parent else 'this build'}")
    parent = open_parent(args.parent) if args.parent else _lib.lib
    g = torch.Generator(device="cuda").manual_seed(k)
    D, H = model(n, p, k, g)
    X8 = draw(D, H, g)
    if args.x_dtype == "u16":   # (through int16, whose copies every torch build has: the counts are below 256)
        X8 = X8.to(torch.int16)
    elif args.x_dtype != "u8":
        X8 = X8.to(torch.float32 if args.x_dtype == "f32" else torch.float64)
    as_x = (lambda T: T.view(torch.uint16)) if args.x_dtype == "u16" else (lambda T: T)
    f64 = dict(dtype=torch.float64, device="cuda")
    bmax = max(sizes)
    Ds = torch.stack([D * (1.0 + b / 100.0) for b in range(bmax)]).contiguous()
    outs = {who: tuple(torch.empty(s, **f64) for s in (n, n, n, (n, k), (n, nt))) for who in ("parent", "single")}
    un = torch.zeros(1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(_lib.lib.espm_spectra_ml_pass_scratch(n, p, k) // 8, **f64)
    bout = tuple(torch.empty(s, **f64) for s in ((bmax, n), (bmax, n), (bmax, n, k), (bmax, n, nt)))
    bun = torch.zeros(bmax, dtype=torch.int64, device="cuda")
    bscratch = torch.empty(_lib.lib.espm_spectra_ml_pass_batch_scratch(n, p, k, bmax) // 8, **f64)
    for layout in ("cm", "pm"):
        X = as_x(X8 if layout == "cm" else X8.t().contiguous())
        fns = {"parent": (lambda: single(parent, X, layout, D, H, outs["parent"], un, scratch), args.calls),
               "single": (lambda: single(_lib.lib, X, layout, D, H, outs["single"], un, scratch), args.calls)}
        for B in sizes:
            fns[f"batch {B}"] = ((lambda B=B: batched(X, layout, Ds[:B], H, tuple(o[:B] for o in bout), bun, bscratch)), max(1, args.calls // B))
        for _ in range(2):
            for fn, _c in fns.values():
                fn()
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(outs["parent"], outs["single"]))
        same_b = all(torch.equal(outs["single"][i], bout[j][0]) for i, j in ((0, 0), (2, 1), (3, 2), (4, 3)))
        t = {who: [] for who in fns}
        for _ in range(args.runs):
            for who, (fn, calls) in fns.items():
                t[who].append(window(fn, calls))
        med = {who: statistics.median(v) for who, v in t.items()}
        say(f"  {layout}: yardstick {med['parent']:.3f} ms (median; {min(t['parent']):.3f} - {max(t['parent']):.3f}, spread "
            f"{100 * (max(t['parent']) / min(t['parent']) - 1):.1f} %); this build's single pass {med['single']:.3f} ms "
            f"({min(t['single']):.3f} - {max(t['single']):.3f}), ratio {med['single'] / med['parent']:.3f}, bit-equal: {same}")
        for B in sizes:
            v = t[f"batch {B}"]
            say(f"      batch of {B}: {med[f'batch {B}']:.3f} ms a call ({min(v):.3f} - {max(v):.3f}), {med[f'batch {B}'] / B:.3f} ms a model, ratio "
                f"{med[f'batch {B}'] / B / med['parent']:.3f} per model; model 0 bit-equal to the single pass: {same_b}; scratch "
                f"{B * scratch.numel() * 8 / 1e6:.0f} MB")
        del X
    del outs, bout, scratch, bscratch, X8, Ds
    torch.cuda.empty_cache()

    if m > 0:
        # ---- end to end: intervals() with the synthetic dictionary of spectra_ml_time.py ---------------------------------------------
        c = torch.arange(n, device="cuda", dtype=torch.float64)[:, None]
        G = torch.exp(-0.5 * ((c - (torch.arange(m, device="cuda", dtype=torch.float64)[None, :] + 0.5) * n / m) / (n / (6.0 * m))) ** 2) + 0.05
        W = torch.rand((m, k), generator=g, device="cuda", dtype=torch.float64) ** 2 + 0.05
        W[1, 2 % k] = W[m - 2, 0] = 0.0   # two entries planted at zero
        W = W * (COUNTS / (G @ W).sum(dim=0, keepdim=True))
        X = draw((G @ W).contiguous(), H, g)
        Gh, Hh = G.cpu().numpy(), H.cpu().numpy()
        for batch in (None, 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = spectra_ml.intervals(X, Gh, Hh, batch=batch)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            say(f"intervals(batch={batch}), dictionary of m = {m}: {len(res['entries'])} tested entries, {res['converged'].size} ends, batch "
                f"{res['batch']}: {total:.2f} s (upload, the count of N and the full fit of {res['n_full_pass']} passes included); "
                f"{int(res['n_pass'].sum())} passes of pinned fits in {res['n_lockstep']} lockstep passes, at most {int(res['n_eval'].max())} "
                f"evaluations an end, all found: {bool(res['converged'].all())}; lower == 0 at {int((res['lower'] == 0).sum())} entries "
                f"(planted: {res['lower'][1, 2 % k]:.3g}, {res['lower'][m - 2, 0]:.3g}; their upper limits {res['upper'][1, 2 % k]:.3g}, "
                f"{res['upper'][m - 2, 0]:.3g})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
