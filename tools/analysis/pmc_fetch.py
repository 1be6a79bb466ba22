#!/usr/bin/env python3
"""FETCH_SIZE of the fused launch from rocprofv3 counter-collection CSVs (a --pmc FETCH_SIZE pass of its own):

    python3 tools/analysis/pmc_fetch.py [--last 20] name=DIR_OR_CSV ...

Per name: the dispatches of mu_fused_ell_kernel in dispatch order, the mean and the range of the counter over the LAST `--last` of them
(the earlier ones are the run-in: the generic first launch and the iterations that fill the last-level cache).  The counter is in KB and
counts half the bytes of a wide coalesced read on gfx950: the second column doubles it."""
import csv
import glob
import os
import sys


def fused_values(path, counter="FETCH_SIZE"):
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*counter_collection.csv"), recursive=True))
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "mu_fused_ell_kernel" in r.get("Kernel_Name", "") and r.get("Counter_Name") == counter:
                    rows.append((int(r["Dispatch_Id"]), float(r["Counter_Value"])))
    per = {}
    for d, v in rows:   # (a counter comes in one row per dimension instance on some stacks: summed per dispatch)
        per[d] = per.get(d, 0.0) + v
    return [per[d] for d in sorted(per)]


def main():
    args = sys.argv[1:]
    last = 20
    if args and args[0] == "--last":
        last, args = int(args[1]), args[2:]
    print(f"FETCH_SIZE per fused launch, mean over the last {last} launches: counter [KB] | x 2 x 1024 [MB] | min .. max [KB] | launches seen")
    for spec in args:
        name, path = spec.split("=", 1)
        v = fused_values(path)
        if not v:
            print(f"{name:16s} no fused launch in {path}")
            continue
        w = v[-last:]
        mean = sum(w) / len(w)
        print(f"{name:16s} {mean:12.1f} | {mean * 2 * 1024 / 1e6:8.1f} | {min(w):.1f} .. {max(w):.1f} | {len(v)}")


if __name__ == "__main__":
    main()
