#!/usr/bin/env python3
"""Is the device code of one set of objects the same, kernel by kernel, as that of another?  For moving kernels between
translation units: the gfx950 code object of every object file is unbundled, and per kernel symbol the disassembly (addresses
stripped, encodings kept) and the kernel's metadata (VGPRs, AGPRs, SGPRs, scratch, LDS, kernarg bytes) are compared as text.

  python3 tools/analysis/kernel_object_diff.py --old-dir OLD/espm_amd/lib --old-units mu_w_step \\
      --new-dir espm_amd/lib --new-units mu_w_accum,mu_w_reduce,mu_w_exchange,mu_w_finish,mu_w_dict > profiles/w_step_split_kernel_diff.txt

Every variant of the library is compared (object prefixes "", "wide_", "wide32_").  Exit status 1 on any difference.  No GPU needed."""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

BIN = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """The gfx950 code object inside an object file's .hip_fatbin section."""
    fat = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    run(f"{BIN}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj)
    targets = [t for t in run(f"{BIN}/clang-offload-bundler", "--list", "--type=o", f"--input={fat}").split() if "gfx950" in t]
    assert len(targets) == 1, (obj, targets)
    out = os.path.join(tmp, os.path.basename(obj) + ".co")
    run(f"{BIN}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={targets[0]}", f"--input={fat}", f"--output={out}")
    return out


def kernels(obj, tmp):
    """{kernel symbol: (metadata text, disassembly text)} of one object; none for a unit of host stubs (no device code at all)."""
    if ".hip_fatbin" not in run(f"{BIN}/llvm-readelf", "-SW", obj):
        return {}
    co = code_object(obj, tmp)
    meta = {}
    for entry in re.split(r"\n  - ", run(f"{BIN}/llvm-readelf", "--notes", co).split("amdhsa.kernels:")[1].split("amdhsa.target:")[0]):
        name = re.search(r"\.name:\s+(\S+)", entry)
        if name:
            found = {f: re.search(re.escape(f) + r":\s+(\d+)", entry) for f in META}
            meta[name.group(1)] = " ".join(f"{f[1:]}={found[f].group(1) if found[f] else '-'}" for f in META)
    end = {}   # where a kernel's code ends (its symbol's size): what follows the last one in the section is padding
    for line in run(f"{BIN}/llvm-readelf", "-sW", co).split("\n"):
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            end[f[7]] = int(f[1], 16) + int(f[2])
    text, cur = {}, None
    for line in run(f"{BIN}/llvm-objdump", "-d", co).split("\n"):
        m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
        addr = re.search(r"// ([0-9A-Fa-f]+):", line)
        if m:
            cur = m.group(1)
            text[cur] = []
        elif cur and addr and int(addr.group(1), 16) < end[cur]:
            text[cur].append(re.sub(r"// [0-9A-Fa-f]+:", "//", line).strip())   # (the address goes; the encoding behind it stays)
    return {k: (meta[k], "\n".join(text.get(k, []))) for k in meta}


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=BIN)
    if not filt or not names:
        return {n: n for n in names}
    return dict(zip(names, subprocess.run([filt], input="\n".join(names), check=True, capture_output=True, text=True).stdout.split("\n")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old-dir", required=True)
    ap.add_argument("--old-units", required=True)
    ap.add_argument("--new-dir", required=True)
    ap.add_argument("--new-units", required=True)
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for prefix in ("", "wide_", "wide32_"):
            sides = []
            for d, units in ((a.old_dir, a.old_units), (a.new_dir, a.new_units)):
                side, twice = {}, []
                for u in units.split(","):
                    os.makedirs(os.path.join(tmp, d.strip("/").replace("/", "_")), exist_ok=True)
                    for k, v in kernels(os.path.join(d, prefix + u + ".o"), os.path.join(tmp, d.strip("/").replace("/", "_"))).items():
                        if k in side:
                            twice.append(k)
                        side[k] = v + (u,)
                sides.append((side, twice))
            (old, _), (new, twice) = sides
            names = demangle(sorted(set(old) | set(new)))
            same = [k for k in old if k in new and old[k][:2] == new[k][:2]]
            print(f"== {prefix or 'narrow_'}: {len(old)} kernels in {a.old_units}, {len(new)} in {a.new_units}; {len(same)} identical (disassembly and metadata)")
            per_unit = {}
            for k in new:
                per_unit[new[k][2]] = per_unit.get(new[k][2], 0) + 1
            print("   per new unit: " + ", ".join(f"{u} {n}" for u, n in per_unit.items()))
            h = hashlib.sha256()
            for k in sorted(new):
                h.update((k + "\n" + new[k][0] + "\n" + new[k][1] + "\n").encode())
            print(f"   sha256 over the new side's kernels (name, metadata, disassembly): {h.hexdigest()}")
            for k in sorted(set(old) - set(new)):
                bad += 1
                print(f"   MISSING  {names[k]}")
            for k in sorted(set(new) - set(old)):
                bad += 1
                print(f"   ADDED    {names[k]} ({new[k][2]})")
            for k in twice:
                bad += 1
                print(f"   TWICE    {names[k]}")
            for k in sorted(set(old) & set(new)):
                if old[k][:2] != new[k][:2]:
                    bad += 1
                    lo, ln = old[k][1].split("\n"), new[k][1].split("\n")
                    nd = sum(1 for x, y in zip(lo, ln) if x != y) + abs(len(lo) - len(ln))
                    print(f"   DIFFERS  {names[k]} ({new[k][2]}): metadata {old[k][0]} -> {new[k][0]}; {len(lo)} -> {len(ln)} lines, {nd} differ")
    print("all kernels identical" if not bad else f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
