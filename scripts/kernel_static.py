#!/usr/bin/env python3
"""Static instruction mix of the kernels in gfx950 assembly files (hipcc ... --cuda-device-only -S -o x.s).

    scripts/kernel_static.py a.s [b.s ...]

Per kernel: code bytes (codeLenInByte), VGPRs, scratch bytes per lane, occupancy, VALU instructions (v_*), IEEE
division expansions (v_div_fixup_f32, one per division) and v_rcp_f32. Nothing is run.
"""
import re
import subprocess
import sys


def kernels(path):
    """name -> figures; a function's instructions run from its label to .Lfunc_end, its resource comments follow"""
    out, cur, body = {}, None, False
    for line in open(path, errors="replace"):
        t = line.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, body = m.group(1), True
            out[cur] = {"valu": 0, "div": 0, "rcp": 0, "kernel": False}
        elif cur is None:
            continue
        elif t.startswith(".Lfunc_end"):
            body = False
        elif body:
            if t.startswith("v_"):
                out[cur]["valu"] += 1
                out[cur]["div"] += t.startswith("v_div_fixup_f32")
                out[cur]["rcp"] += t.startswith("v_rcp_f32")
            elif t.startswith(".end_amdhsa_kernel"):
                out[cur]["kernel"] = True
        else:
            for key, pat in (("code", r"; codeLenInByte = (\d+)"), ("vgpr", r"; NumVgprs: (\d+)"),
                             ("scratch", r"; ScratchSize: (\d+)"), ("occ", r"; Occupancy: (\d+)")):
                m = re.match(pat, t)
                if m:
                    out[cur][key] = int(m.group(1))
    return {k: v for k, v in out.items() if v["kernel"] and "code" in v}


def main():
    for path in sys.argv[1:]:
        ks = kernels(path)
        names = sorted(ks)
        dm = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
        print(f"# {path}")
        for n, d in zip(names, dm):
            v = ks[n]
            short = re.sub(r"^void nh\w*::", "", d).split("(")[0]
            print(f"code={v['code']:7d} vgpr={v.get('vgpr', -1):3d} scratch={v.get('scratch', -1):4d} occ={v.get('occ', -1)} "
                  f"valu={v['valu']:6d} div={v['div']:4d} rcp={v['rcp']:4d}  {short}")


if __name__ == "__main__":
    main()
