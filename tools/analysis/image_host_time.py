"""What a call of an image analysis costs from call to result, upload included, in two trees: the record behind giving the analysis
modules one upload and one resident-image type (profiles/image_host_time.log).  The kernels are the same library in both trees;
what could move is the host side - the checks, the upload, the read-back.

    python tools/analysis/image_host_time.py run OUT.json [--root TREE] [--size n,nx,ny] [--calls 3]
    python tools/analysis/image_host_time.py report PARENT.json PARENT_AGAIN.json NEW.json [--more RUN.json ...] [--out profiles/image_host_time.log]

``run`` imports espm_amd from TREE (default: this tree) and times, at the headline image of the ``*_time.py`` tools (2048 channels x
512^2 pixels, k = 5, 500 counts per pixel, 8-bit, channel-major), with X as a host array and as a device-resident tensor:

  measures.pixel_diagnostics(X, D, H, simplex_H=True);   marginals.pixel_maps(X, 8 windows of 20 channels), no model;
  attribution.expected(X, D, H);   binning.binning_risk(X, (ny, nx)), the default 256 candidates;   presence.presence(X, D, "newton").

Every call is made once unmeasured and then --calls times between ``torch.cuda.synchronize()`` and the wall clock; the median and
min - max go to OUT.json.  ``report`` takes two runs of the parent and one of the new tree: the margin is the parent's own spread
between its two runs, |a - b| of the medians, and a row of the new tree is "within" when its median is not above the slower parent
run by more than that.  Two runs are a thin estimate of a spread: ``--more`` lists the medians of further runs of either tree under
the three columns, for a row that falls outside."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(out, size, calls):
    import numpy as np
    import torch

    import espm_amd   # (first: the tools imported below put this tree in front of sys.path, and take the package as it is loaded)
    from espm_amd import attribution, binning, marginals, measures, presence
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import pixel_diagnostics_time as pdt
    n, nx, ny = size
    p, k = nx * ny, 5
    g = torch.Generator(device="cuda").manual_seed(k)
    Dd, Hd = pdt.model(n, p, k, g)
    Xdev = pdt.draw(Dd, Hd, g)
    Xhost, D, H = Xdev.cpu().numpy(), Dd.cpu().numpy(), Hd.cpu().numpy()
    del Dd, Hd
    U = marginals.window_weights(n, [(a, a + 20) for a in range(100, 100 + 8 * 200, 200)])
    cases = [("pixel_diagnostics", lambda X: measures.pixel_diagnostics(X, D, H, simplex_H=True)),
             ("pixel_maps, 8 windows of 20", lambda X: marginals.pixel_maps(X, U)),
             ("attribution.expected", lambda X: attribution.expected(X, D, H)),
             ("binning_risk, 256 candidates", lambda X: binning.binning_risk(X, (ny, nx))),
             ("presence, newton", lambda X: presence.presence(X, D, method="newton"))]
    rows = {}
    for name, call in cases:
        for where, X in (("host", Xhost), ("device", Xdev)):
            call(X)
            ms = []
            for _ in range(calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(X)
                torch.cuda.synchronize()
                ms.append(1e3 * (time.perf_counter() - t0))
            rows[f"{name} | {where}"] = dict(median=float(np.median(ms)), min=min(ms), max=max(ms))
            print(f"{name:30s} {where:6s}: {np.median(ms):9.2f} ms ({min(ms):.2f} - {max(ms):.2f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(tree=os.path.dirname(os.path.abspath(espm_amd.__file__)), size=[n, nx, ny], calls=calls,
                       device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


def report(files, more, out):
    runs = [json.load(open(f)) for f in files]
    n, nx, ny = runs[0]["size"]
    cell = lambda r: f"{r['median']:9.2f} ({r['min']:8.2f} -{r['max']:9.2f})"   # noqa: E731
    lines = [f"image_host_time: call to result, upload and read-back included, ms: median (min - max) of {runs[0]['calls']} calls after one "
             f"unmeasured; {n} channels x {nx} x {ny} pixels, k = 5, uint8 channel-major, {runs[0]['device']}",
             f"parent: {files[0]}, parent again: {files[1]}, new: {files[2]}; margin = |parent - parent again| of the medians", "",
             f"{'call':30s} {'X':6s} {'parent':>30s} {'parent again':>30s} {'new':>30s} {'margin':>8s}  new against the slower parent run"]
    outside = 0
    for key in runs[0]["rows"]:
        a, b, c = (r["rows"][key] for r in runs)
        margin = abs(a["median"] - b["median"])
        over = c["median"] - max(a["median"], b["median"])
        ok = over <= margin
        outside += not ok
        name, where = key.split(" | ")
        lines.append(f"{name:30s} {where:6s} {cell(a):>30s} {cell(b):>30s} {cell(c):>30s} {margin:8.2f}  {over:+9.2f} ms: "
                     f"{'within' if ok else 'OUTSIDE'}")
    lines += ["", f"RESULT: {'every row within the parent spread' if not outside else f'{outside} rows outside the parent spread'}"]
    if more:
        extra = [json.load(open(f)) for f in more]
        names = [os.path.splitext(os.path.basename(f))[0] for f in more]
        lines += ["", "medians of further runs in the same session, ms (in the order they were made):",
                  f"{'call':30s} {'X':6s} " + " ".join(f"{v:>14s}" for v in names)]
        for key in runs[0]["rows"]:
            name, where = key.split(" | ")
            lines.append(f"{name:30s} {where:6s} " + " ".join(f"{r['rows'][key]['median']:14.2f}" for r in extra))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("out")
    r.add_argument("--root", default=HERE)
    r.add_argument("--size", default="2048,512,512")
    r.add_argument("--calls", type=int, default=3)
    c = sub.add_parser("report")
    c.add_argument("files", nargs=3)
    c.add_argument("--more", nargs="*", default=[])
    c.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.cmd == "report":
        return report(args.files, args.more, args.out)
    sys.path.insert(0, os.path.abspath(args.root))
    run(args.out, tuple(int(v) for v in args.size.split(",")), args.calls)


if __name__ == "__main__":
    main()
