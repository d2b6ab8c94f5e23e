"""Msamples/s of the av integrator in both render modes.

    python scripts/av_rate.py [--spp 16] [--repeats 5] [--out FILE]

Two scenes at 1024 x 1024: the Cornell box (shallow tree) and scenegen.bumpy_cbox_xml at the C3 mesh size (1000 x 250,
498k triangles: a deep tree on the wide traversal), both with <integrator type="av"> and length 0.2, a tenth of the
box's extent. Per scene the two modes alternate, `repeats` timed renders each after one warm-up render of the same
shape; a render is timed by the host clock from the call to the end of nh_synchronize. The framebuffers of the two modes
are compared bit for bit at the size timed. One JSON line per scene.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "optix-renderer_amd"))


def main():
    import nori_hip as nh
    import scenegen
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--length", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    nh.configure_runtime()
    assert nh.device_count() > 0, "no GPU visible"
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        scenes = [("cbox", scenegen.cbox_xml(tmp, "c2")), ("bumpy_1000x250", scenegen.bumpy_cbox_xml(tmp, 1000, 250)[0])]
        for name, xml in scenes:
            s = nh.Scene(xml)
            s.set_resolution(args.size, args.size)
            s.set_integrator(nh.INTEGRATOR_AV)
            s.set_av_params(args.length)
            b = nh.Bvh(s)
            ctx = nh.Context(0)
            ctx.upload(s, b)
            n = args.size * args.size * args.spp
            modes = {"megakernel": nh.MODE_MEGAKERNEL, "wavefront": nh.MODE_WAVEFRONT}
            fbs, times = {}, {k: [] for k in modes}
            for k, m in modes.items():  # warm-up, and the outputs to compare
                ctx.render(0, args.spp, seed=1, mode=m, traversal=nh.TRAVERSAL_ORDERED, clear=True)
                ctx.synchronize()
                fbs[k] = ctx.framebuffer()
            for _ in range(args.repeats):
                for k, m in modes.items():
                    t0 = time.perf_counter()
                    ctx.render(0, args.spp, seed=1, mode=m, traversal=nh.TRAVERSAL_ORDERED, clear=True)
                    ctx.synchronize()
                    times[k].append(time.perf_counter() - t0)
            rec = {"scene": name, "size": args.size, "spp": args.spp, "length": args.length,
                   "bvh_max_depth": int(b.desc.max_depth), "wide": ctx.stats()["node_bytes"] != 64,
                   "identical": bool(np.array_equal(fbs["megakernel"].view(np.uint32), fbs["wavefront"].view(np.uint32))),
                   "occluded_share": float(1.0 - fbs["megakernel"][..., 0].sum() / fbs["megakernel"][..., 3].sum())}
            for k in modes:
                t = np.array(times[k])
                rec[k] = {"msamples_per_s_median": n / float(np.median(t)) / 1e6, "msamples_per_s_min": n / float(t.max()) / 1e6,
                          "msamples_per_s_max": n / float(t.min()) / 1e6, "seconds": [round(float(x), 5) for x in t]}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
