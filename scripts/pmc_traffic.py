"""Record HBM bytes per launch of one kernel from a scripts/pmc.sh run into profiles/pmc_traffic.json.

usage: python scripts/pmc_traffic.py PMC_DIR WORKLOAD_KEY KERNEL_SUBSTRING [--merge]
PMC_DIR: the pmc_TAG directory a scripts/pmc.sh or scripts/pmc_groups.sh run wrote its passes to.
FETCH_SIZE (KB) is doubled (gfx950 reports half the bytes of wide coalesced reads,
MI355X_MICROARCH.md HBM section); WRITE_SIZE (KB) is taken as is. Both are averaged over the
kernel's dispatches, like the bench's achieved bytes per launch.
The record names the full kernel instantiation the counters came from (one distinct kernel name must match
KERNEL_SUBSTRING) and the build it ran: lib_sha16, the first 16 hex digits of the SHA-256 of the library the passes
loaded (NH_LIB_PATH, else optix-renderer_amd/lib/libnori_hip.so). bench.py uses a record only for that same build.
--merge: a stage that runs several instantiations (the diffuse area-light bounce kernels: one for bounce 0, one for
the later bounces) is recorded as one stage -- every dispatch of every kernel that matches counts, as in the bench's
per-launch average; `kernel` lists them.
Passes of the instruction-mix and instruction-fetch groups (scripts/pmc_groups.sh with e.g.
  "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_FLAT SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SMEM"
  "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_IFETCH SQ_BUSY_CYCLES GRBM_GUI_ACTIVE"
  "SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE")
are recorded per launch under `counters`, with the derived icache_hit_rate, lds_wait_frac and inst_wait_frac. A counter
the device does not have never appears in the CSVs and is listed under `counters_missing`.
"""
import hashlib
import csv
import glob
import json
import os
import sys
from collections import defaultdict

root, key, pat = sys.argv[1:4]
merge = "--merge" in sys.argv[4:]
# instruction mix, waits and instruction fetch (all optional: recorded when a pass collected them)
EXTRA = ("SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_FLAT", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_INSTS_SMEM",
         "SQ_WAIT_INST_ANY", "SQ_WAIT_INST_LDS", "SQ_IFETCH", "SQ_BUSY_CYCLES", "SQC_ICACHE_REQ", "SQC_ICACHE_HITS",
         "SQC_ICACHE_MISSES", "SQC_ICACHE_MISSES_DUPLICATE")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = os.environ.get("NH_LIB_PATH") or os.path.join(REPO, "optix-renderer_amd", "lib", "libnori_hip.so")
lib_sha16 = hashlib.sha256(open(lib, "rb").read()).hexdigest()[:16]
vals = defaultdict(list)
names = set()
for f in glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        if pat in r["Kernel_Name"]:
            names.add(r["Kernel_Name"])
        if pat in r["Kernel_Name"] and r["Counter_Name"] in ("FETCH_SIZE", "WRITE_SIZE", "SQ_INSTS_VALU",
                                                             "GRBM_GUI_ACTIVE", "SQ_WAIT_ANY", "SQ_WAVE_CYCLES",
                                                             "SQ_ACTIVE_INST_VALU", "VALUBusy", "VALUUtilization",
                                                             "TCC_HIT_sum", "TCC_MISS_sum") + EXTRA:
            vals[r["Counter_Name"]].append(float(r["Counter_Value"]))
if len(names) != 1 and not (merge and names):
    sys.exit(f"pmc_traffic: {len(names)} distinct kernels match {pat!r}: {sorted(names)}")
kernel = "; ".join(sorted(names))
if not vals["FETCH_SIZE"] or not vals["WRITE_SIZE"]:
    sys.exit(f"pmc_traffic: no FETCH_SIZE / WRITE_SIZE pass under {root}")
fetch = sum(vals["FETCH_SIZE"]) / len(vals["FETCH_SIZE"]) * 2 * 1024  # x2: gfx950 FETCH_SIZE (HBM section)
write = sum(vals["WRITE_SIZE"]) / len(vals["WRITE_SIZE"]) * 1024
out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pmc_traffic.json")
data = json.load(open(out)) if os.path.exists(out) else {}
data[key] = {"kernel": kernel, "lib_sha16": lib_sha16, "hbm_bytes_per_launch": int(fetch + write), "read_bytes_per_launch": int(fetch),
             "write_bytes_per_launch": int(write), "dispatches": len(vals["FETCH_SIZE"]),
             "source": f"rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes), {os.path.basename(root)}"}
avg = lambda k: sum(vals[k]) / len(vals[k]) if vals[k] else None  # noqa: E731
if avg("SQ_INSTS_VALU") and avg("GRBM_GUI_ACTIVE"):
    # VALU issue: one wave64 VALU instruction per cycle per CU -- each takes its SIMD one quad-cycle
    # (SQ_ACTIVE_INST_VALU, in quad-cycles, ~ SQ_INSTS_VALU: recorded below), 4 SIMDs per CU;
    # GRBM_GUI_ACTIVE sums the 8 XCDs' busy cycles
    cycles = avg("GRBM_GUI_ACTIVE") / 8
    data[key]["valu_insts_per_launch"] = int(avg("SQ_INSTS_VALU"))
    data[key]["valu_issue_frac"] = round(avg("SQ_INSTS_VALU") / (cycles * 256), 3)
if avg("SQ_ACTIVE_INST_VALU") and avg("SQ_INSTS_VALU"):
    data[key]["quad_cycles_per_valu_inst"] = round(avg("SQ_ACTIVE_INST_VALU") / avg("SQ_INSTS_VALU"), 3)
if avg("VALUBusy") is not None:
    data[key]["valu_busy_pct"] = round(avg("VALUBusy"), 1)
if avg("VALUUtilization") is not None:
    data[key]["valu_utilization_pct"] = round(avg("VALUUtilization"), 1)
if avg("TCC_HIT_sum") is not None and avg("TCC_MISS_sum") is not None:
    data[key]["l2_hit_rate"] = round(avg("TCC_HIT_sum") / max(avg("TCC_HIT_sum") + avg("TCC_MISS_sum"), 1.0), 3)
if avg("SQ_WAIT_ANY") and avg("SQ_WAVE_CYCLES"):
    data[key]["wait_frac"] = round(avg("SQ_WAIT_ANY") / avg("SQ_WAVE_CYCLES"), 3)
extra = {k: int(avg(k)) for k in EXTRA if avg(k) is not None}
if extra:
    data[key]["counters"] = extra
    data[key]["counters_missing"] = sorted(k for k in EXTRA if k not in extra)
    if extra.get("SQC_ICACHE_REQ"):
        data[key]["icache_hit_rate"] = round(extra.get("SQC_ICACHE_HITS", 0) / extra["SQC_ICACHE_REQ"], 4)
    if avg("SQ_WAVE_CYCLES"):
        if "SQ_WAIT_INST_LDS" in extra:
            data[key]["lds_wait_frac"] = round(extra["SQ_WAIT_INST_LDS"] / avg("SQ_WAVE_CYCLES"), 3)
        if "SQ_WAIT_INST_ANY" in extra:
            data[key]["inst_wait_frac"] = round(extra["SQ_WAIT_INST_ANY"] / avg("SQ_WAVE_CYCLES"), 3)
json.dump(data, open(out, "w"), indent=1, sort_keys=True)
print(key, data[key])
