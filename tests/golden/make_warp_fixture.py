"""Regenerates tests/golden/warp_runs.json on the CPU, from the restatement alone (warp_refs; no GPU, a few minutes).

    python tests/golden/make_warp_fixture.py

WarpTest::runTest (src/utils/warptest.cpp:439-562) for the twelve warp types the HIP path runs, at the reference's own
table (51 x 51 cells, 51 x 102 beyond None and Disk, 1000 points per cell) and g++'s draw order. Digests, not tables:
per type the sliders and the mapped parameter, sum(obs), the points skipped for weight 0 and left out for a NaN
coordinate, a SHA-256 of the counts as little-endian uint32, 16 cells of obs and exp (exp as hex doubles), exp_sum,
the pdf evaluations in all, and the verdict: kind, dof, pooled cells, statistic, p-value. Prints one line per type.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "optix-renderer_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

# name (nori_hip.WARP_NAMES): (parameter slider, angle slider). The Henyey-Greenstein sliders keep |g| at 0.3: towards
# |g| = 1 squareToHenyeyGreenstein returns NaN points (1 - cos^2 rounds below zero), which the reference cannot bin
SLIDERS = {"none": (0.5, 0.5), "disk": (0.5, 0.5), "sphere": (0.5, 0.5), "spherevol": (0.5, 0.5),
           "spherecap": (0.5, 0.5), "hemisphere": (0.5, 0.5), "cosinehemisphere": (0.5, 0.5), "beckmann": (0.5, 0.5),
           "henyeygreenstein": (0.65, 0.5), "microfacet": (0.5, 0.7), "isophase": (0.5, 0.5), "anisophase": (0.35, 0.5)}


def sampled_cells(n_cells: int):
    return [(2 * k + 1) * n_cells // 32 for k in range(16)]


def build(yres: int = 0, xres: int = 0) -> dict:
    """The fixture's content; yres = xres = 0: the reference's own table, else that one with 1000 points per cell."""
    import nori_hip as nh
    import warp_refs as wr
    runs = {}
    for name, (ps, angle) in SLIDERS.items():
        t = nh.WARP_NAMES.index(name)
        r = wr.execute(t, ps, angle, True, xres, yres, 1000 * xres * yres)
        cells = sampled_cells(r["xres"] * r["yres"])
        runs[name] = {"parameter_slider": ps, "angle_slider": angle, "parameter": float(r["parameter"]).hex(),
                      "xres": r["xres"], "yres": r["yres"], "sample_count": r["sample_count"],
                      "obs_sum": int(r["obs_sum"]), "skipped": r["skipped"], "nan_points": r["nan_points"],
                      "obs_sha256": wr.digest(r["obs"]), "cells": cells, "obs": [int(r["obs"][c]) for c in cells],
                      "exp": [float(r["exp"][c]).hex() for c in cells], "exp_sum": float(r["exp_sum"]).hex(),
                      "evals": int(r["evals"].sum()), "kind": r["kind"], "accepted": bool(r["accepted"]),
                      "dof": r["dof"], "pooled_cells": r["pooled_cells"], "statistic": r["statistic"],
                      "p_value": r["p_value"]}
        print(f"{name}: parameter {float(r['parameter']):.6g}, {r['yres']}x{r['xres']}, obs_sum {int(r['obs_sum'])}, skipped "
              f"{r['skipped']}, NaN {r['nan_points']}, exp_sum {r['exp_sum']:.6f}, evaluations {int(r['evals'].sum())}, "
              f"{chi2_kind(r['kind'])}, statistic {r['statistic']:.6g}, dof {r['dof']}, pooled {r['pooled_cells']}, "
              f"p {r['p_value']:.6g}", flush=True)
    return {"draw_order": "rtl", "runs": runs}


def chi2_kind(kind: int) -> str:
    return ("accepted", "rejected: p-value", "rejected: expected frequency 0", "rejected: degrees of freedom")[kind]


def main():
    out = build()
    with open(os.path.join(HERE, "warp_runs.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
