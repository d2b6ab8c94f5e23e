#!/usr/bin/env python3
"""Rate of the adaptive sampler's render loop on one GPU, beside the independent sampler at the same sample count.

    scripts/adaptive_rate.py [--scene XML] [--width W --height H] [--samples N] [--runs R]

Default scene: the reference's scenes/project/disney/disney-test.xml from tests/golden/adaptive_scenes.json.gz (its
mesh and envmap are the fixture's stand-ins) at its own size (800x800) and outer sample count (100). A run renders
the scene once through the adaptive loop and once with the independent sampler (megakernel) at the sample count per
pixel that places as many samples in total, rounded up; the runs of the two are interleaved. Prints one JSON line: the
median samples placed per second of wall time of each, and the adaptive loop's passes.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "optix-renderer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--samples", type=int)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()

    import adaptive_refs as ar
    import nori_hip as nh
    nh.configure_runtime()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.scene or os.path.join(ar.materialize(tmp), ar.DISNEY_TEST_XML)
        s, t = nh.Scene(path), nh.Scene(path)
    for x in (s, t):
        if a.width or a.height:
            x.set_resolution(a.width or x.width, a.height or x.height)
    if s.desc.sampler != nh.SAMPLER_ADAPTIVE:
        s.set_sampler(nh.SAMPLER_ADAPTIVE, 2)
    t.set_sampler(nh.SAMPLER_INDEPENDENT)
    n = a.samples or s.spp
    ca, ci = nh.Context(0), nh.Context(0)
    ca.upload(s, nh.Bvh(s))
    ci.upload(t, nh.Bvh(t))

    def adaptive(seed):
        t0 = time.perf_counter()
        ca.render(0, n, seed=seed, clear=True)
        ca.synchronize()
        return time.perf_counter() - t0

    adaptive(0)  # warm-up; also tells the independent render its sample count
    st = ca.adaptive_stats()
    spp = -(-st["total_samples"] // (s.width * s.height))

    def independent(seed):
        t0 = time.perf_counter()
        ci.render(0, spp, seed=seed, clear=True, traversal=nh.TRAVERSAL_ORDERED)
        ci.synchronize()
        return time.perf_counter() - t0

    independent(0)
    ra, ri, placed = [], [], []
    for i in range(a.runs):
        dt = adaptive(1 + i)
        placed.append(ca.adaptive_stats()["total_samples"])
        ra.append(placed[-1] / dt)
        ri.append(s.width * s.height * spp / independent(1 + i))
    st = ca.adaptive_stats()
    print(json.dumps({"scene": os.path.basename(path), "width": s.width, "height": s.height, "outer_samples": n,
                      "runs": a.runs, "adaptive_samples_placed": placed, "adaptive_passes": st["passes"],
                      "adaptive_max_passes": st["max_passes"], "n_blocks": st["n_blocks"],
                      "adaptive_msamples_per_s": statistics.median(ra) / 1e6, "independent_spp": spp,
                      "independent_msamples_per_s": statistics.median(ri) / 1e6}))


if __name__ == "__main__":
    main()
