#!/usr/bin/env python3
"""Kernel resource usage from a build log made with EXTRA_HIP=-Rpass-analysis=kernel-resource-usage.

    make clean && make EXTRA_HIP=-Rpass-analysis=kernel-resource-usage lib 2> build.log
    scripts/kernel_resources.py build.log                 # one line per kernel
    scripts/kernel_resources.py parent.log branch.log     # kernels of both: differences; kernels only in the second: listed
    scripts/kernel_resources.py a.log,b.log ...           # one build's logs merged

Compared per kernel (mangled name): VGPRs, AGPRs, scratch bytes per lane, LDS bytes per block, occupancy, SGPR and
VGPR spills.
"""
import re
import subprocess
import sys

FIELDS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "lds"),
          ("Occupancy [waves/SIMD]", "occ"), ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill")]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = out.setdefault(body.split(":", 1)[1].strip(), {})
            continue
        for label, key in FIELDS:
            if cur is not None and body.startswith(label + ":"):
                cur[key] = int(body.rsplit(":", 1)[1])
    # kernels only (device functions report no occupancy); a record cut up by a parallel build's interleaved output
    # is dropped rather than trusted
    return {k: v for k, v in out.items() if "occ" in v and len(v) == len(FIELDS)}


def parse_all(paths):
    """Several logs of one build, comma-separated: the first complete record of a kernel wins (a serial rebuild of one
    object fills what a parallel build's log garbled)."""
    out = {}
    for p in paths.split(","):
        for k, v in parse(p).items():
            out.setdefault(k, v)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def row(v):
    return " ".join(f"{k}={v.get(k, '?')}" for _, k in FIELDS)


def main():
    if len(sys.argv) == 2:
        ks = parse_all(sys.argv[1])
        dm = demangle(sorted(ks))
        for n in sorted(ks):
            print(f"{row(ks[n])}  {dm[n]}")
        return 0
    a, b = parse_all(sys.argv[1]), parse_all(sys.argv[2])
    dm = demangle(sorted(set(a) | set(b)))
    both = sorted(set(a) & set(b))
    diff = [n for n in both if a[n] != b[n]]
    print(f"{len(both)} kernels in both builds, {len(diff)} with different resources")
    for n in diff:
        print(f"  DIFF {dm[n]}\n    first : {row(a[n])}\n    second: {row(b[n])}")
    gone = sorted(set(a) - set(b))
    print(f"{len(gone)} kernels only in the first build")
    for n in gone:
        print(f"  {dm[n]}")
    new = sorted(set(b) - set(a))
    print(f"{len(new)} kernels only in the second build")
    for n in new:
        print(f"  {row(b[n])}  {dm[n]}")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
