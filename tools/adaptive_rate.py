#!/usr/bin/env python3
"""Adaptive sampling against fixed samples per pixel (prt_render_adaptive vs prt_render_spp), on the MI355X.

For each scene: a reference render (prt_render_spp at --ref-spp with other seeds), fixed renders at 64 / 256 / 1024 spp, and adaptive
renders (min 16, max 1024, rel_err 0.1 / 0.05 / 0.02) with the live-pixel lists on and off.  Per render: wall time, mean spp, the pixels
frozen by convergence and by max_spp, G segments/s, the live lanes of the list launches, RMSE against the reference.  The headline: wall
time to reach the RMSE of fixed 1024 spp, fixed against adaptive.  One JSON document on stdout (and into --out).

    python tools/adaptive_rate.py [--width 1920 --height 1080] [--scenes cornell_diffuse,cornell_roughdiel] [--out profiles/r05_adaptive.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scenes", default="cornell_diffuse,cornell_roughdiel")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--fixed", default="64,256,1024")
    ap.add_argument("--rel", default="0.1,0.05,0.02")
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
    from conftest import VARIANTS, variant_camera, variant_config
    W, H = a.width, a.height
    doc = {"width": W, "height": H, "ref_spp": a.ref_spp, "min_spp": a.min_spp, "max_spp": a.max_spp, "build_id": prt.build_id(), "scenes": {}}
    for variant in a.scenes.split(","):
        scene_json, phase, use_env = VARIANTS[variant]
        scene = prt.HostScene(scene_json)
        cfg = variant_config(scene, variant)
        cfg.phase_function = phase
        r = prt.Renderer(cfg, device=0)
        r.upload_scene(scene)
        if use_env:
            r.upload_envmap(prt.make_sky(64, 32))
        r.set_camera(variant_camera(prt, variant, W, H))
        r.resize(W, H)

        def timed(fn):
            r.reset()
            r.synchronize()
            t0 = time.perf_counter()
            fn()
            r.synchronize()
            return time.perf_counter() - t0

        ref_seeds = prt.seed_pairs(a.ref_spp * 16 + 64, first_frame=1000003)
        t_ref = timed(lambda: r.render_spp(a.ref_spp, ref_seeds))
        ref = r.read_framebuffer()[..., :3].astype(np.float64)
        seeds = prt.seed_pairs(a.max_spp * 16 + 64)

        def measure(t, extra):
            img = r.read_framebuffer()[..., :3].astype(np.float64)
            st = r.read_state()
            c = r.counts()
            n = st["samples"]
            row = {"wall_s": round(t, 4), "mean_spp": round(float(n.mean()), 2), "gseg_per_s": round(c.segments / t / 1e9, 3),
                   "rmse": float(np.sqrt(np.mean((img - ref) ** 2)))}
            row.update(extra(n))
            return row

        out = {"reference_s": round(t_ref, 3), "fixed": {}, "adaptive": {}}
        for spp in [int(x) for x in a.fixed.split(",")]:
            t = timed(lambda: r.render_spp(spp, seeds))
            out["fixed"][str(spp)] = measure(t, lambda n: {})
        for rel in [float(x) for x in a.rel.split(",")]:
            for compact in (1, 0):
                r.set_option("compact", compact)
                t = timed(lambda: r.render_adaptive(seeds, a.min_spp, a.max_spp, rel, 0.0))
                rep = r.adaptive_report()

                def extra(n):
                    return {"frozen_by_convergence": round(float((n < a.max_spp).mean()), 4), "frozen_by_max_spp": round(float((n >= a.max_spp).mean()), 4),
                            "launches": r.stats().launches, "tile_launches": rep.tile_launches, "list_launches": rep.list_launches,
                            "list_builds": rep.list_builds,
                            "list_live_lane_fraction": round(rep.list_live_lanes / rep.list_lanes, 4) if rep.list_lanes else None}
                out["adaptive"]["rel%g_compact%d" % (rel, compact)] = measure(t, extra)
        r.set_option("compact", 1)
        target = out["fixed"].get("1024")
        if target:
            ok = [(v["wall_s"], k) for k, v in out["adaptive"].items() if v["rmse"] <= target["rmse"]]
            out["headline"] = {"fixed_1024_rmse": target["rmse"], "fixed_1024_wall_s": target["wall_s"],
                               "fastest_adaptive_at_or_below_that_rmse": (min(ok)[1] if ok else None),
                               "its_wall_s": (min(ok)[0] if ok else None)}
        doc["scenes"][variant] = out
        r.close()
        print(json.dumps({variant: out}), file=sys.stderr, flush=True)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
