#!/usr/bin/env python3
"""Render rate of a Disney scene on one GPU.

    scripts/disney_rate.py [--scene XML] [--width W --height H] [--spp N] [--mode wavefront|megakernel]
                           [--steps K] [--warmup W] [--png OUT.png]

Default scene: the reference's scenes/project/disney/disney-validation-blender.xml from
tests/golden/disney_scenes.json.gz at its own size (1024x1024) and sample count (512 spp). Each step renders the whole
image; the rate is camera samples per second of wall time over the timed steps, and the kernel split comes from
nh_get_stats over the same steps. Prints one JSON line.
"""
import argparse
import json
import os
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
    ap.add_argument("--spp", type=int)
    ap.add_argument("--mode", choices=["wavefront", "megakernel"], default="wavefront")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--png")
    a = ap.parse_args()

    import disney_scenes as dz
    import nori_hip as nh
    nh.configure_runtime()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.scene or os.path.join(dz.materialize(tmp), dz.VALIDATION_XML)
        s = nh.Scene(path)
    if a.width or a.height:
        s.set_resolution(a.width or s.width, a.height or s.height)
    spp = a.spp or s.spp
    b = nh.Bvh(s)
    c = nh.Context(0)
    c.upload(s, b)
    mode = nh.MODE_WAVEFRONT if a.mode == "wavefront" else nh.MODE_MEGAKERNEL

    def step(i):
        c.render(0, spp, seed=i, clear=True, mode=mode, traversal=nh.TRAVERSAL_ORDERED)
        c.synchronize()
    for i in range(a.warmup):
        step(i)
    c.reset_stats()
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(a.warmup + i)
    dt = time.perf_counter() - t0
    st = c.stats()
    samples = s.width * s.height * spp * a.steps
    kern = {k: st[k] for k in ("kernel_ms_path", "kernel_ms_shade", "kernel_ms_extend", "kernel_ms_shadow",
                               "kernel_ms_tail", "kernel_ms_splat")}
    # wavefront: kernel_ms_path is the sum of the path-tracing kernels (shade + extend + shadow + tail)
    total = st["kernel_ms_path"] + st["kernel_ms_splat"]
    d = s.desc
    out = {"scene": os.path.basename(path), "width": s.width, "height": s.height, "spp": spp, "mode": a.mode,
           "steps": a.steps, "seconds": dt, "msamples_per_s": samples / dt / 1e6,
           "bsdf_types": sorted({d.bsdfs[d.shapes[i].bsdf].type for i in range(d.n_shapes)}),
           "fused_bounce": st["fused_bounce"], "kernel_ms": kern,
           # with the fused bounce kernels the bounce's time is kernel_ms_shade (nh_render_stats::fused_bounce)
           "bounce_or_shade_share": (st["kernel_ms_shade"] / total) if total else None,
           "invalid_samples": st["invalid_samples"]}
    if a.png:
        nh.write_png(a.png, nh.to_rgb(c.framebuffer(), s.border))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
