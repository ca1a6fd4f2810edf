#!/usr/bin/env python3
"""Pixel filters (prt_set_pixel_filter) on the MI355X: what antialiasing costs and what it does to the edges.

1. Throughput at the headline configuration of bench.py (scenes/cornell_diffuse, 1920x1080, 1024 spp, bench.py's seeds) for NONE, box, tent and
   Blackman-Harris: --steps timed renders of each after one warm-up, the kinds interleaved (A B C D A B C D ...) so that clock drift hits all of
   them alike; the median Msamples/s and the kernel variant each ran.
2. Silhouettes: on --edge-scene (an open box under the sky map: edges against the background) at --edge-width x --edge-height, the RMSE of the
   silhouette pixels -- guide coverage at K = 16 (unfiltered guides) strictly between 0 and 1 -- against a --ref-spp render of the same filter,
   at 16, 64 and 256 spp.
3. The same through prt_render_adaptive (min 16, max 256 paths, rel_err 0.05): the mean paths of silhouette pixels and of the others, and the
   silhouette RMSE -- whether the edge pixels now draw samples.
Pixels that are not finite in either picture are counted and left out of the RMSE (round 8: 1 and 2 pixels of the 4096-spp references under
tent and Blackman-Harris, none in the unfiltered ones; not yet explained).  One JSON document on stdout (and into --out).

    python tools/filter_rate.py [--steps 3] [--out profiles/r08_pixel_filter.json]
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

KINDS = ["none", "box", "tent", "blackman-harris"]


def throughput(prt, W, H, spp, steps):
    scene = prt.HostScene("cornell_diffuse.json")
    cfg = scene.config()
    seeds = prt.seed_pairs(max(64, spp * max(cfg.max_bounces, 8) + 64))      # (bench.py's)
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    r.set_camera(prt.default_camera(W, H))
    r.resize(W, H)
    times = {k: [] for k in KINDS}
    variant = {}
    for rep in range(steps + 1):
        for kind in KINDS:
            r.set_pixel_filter(kind)
            r.synchronize()
            t0 = time.perf_counter()
            r.render_spp(spp, seeds)
            r.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                times[kind].append(dt)
            variant[kind] = r.kernel_variant()
    r.close()
    out = {}
    for kind in KINDS:
        med = float(np.median(times[kind]))
        out[kind] = {"msamples_per_s": round(W * H * spp / med / 1e6, 2), "median_s": round(med, 4), "times_s": [round(t, 4) for t in times[kind]],
                     "variant": variant[kind]}
    for kind in KINDS[1:]:
        out[kind]["vs_none"] = round(out[kind]["msamples_per_s"] / out["none"]["msamples_per_s"], 4)
    return out


def edges(prt, scene_json, W, H, ref_spp):
    scene = prt.HostScene(scene_json)
    cfg = scene.config()
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    r.upload_envmap(prt.make_sky(1024, 512))
    r.set_camera(prt.default_camera(W, H))
    r.resize(W, H)
    nf = lambda spp: spp * max(cfg.max_bounces, 8) + 64
    r.render_guides(16)
    cov = r.read_guides()[..., 3]
    sil = (cov > 0) & (cov < 1)
    out = {"silhouette_pixels": int(sil.sum()), "pixels": W * H}

    def rmse(img, ref, mask):
        ok = mask & np.isfinite(img).all(-1) & np.isfinite(ref).all(-1)
        return round(float(np.sqrt(np.mean((img[ok] - ref[ok]) ** 2))), 5)

    for kind in KINDS:
        r.set_pixel_filter(kind)
        r.render_spp(ref_spp, prt.seed_pairs(nf(ref_spp), first_frame=1000001))
        ref = r.read_framebuffer()[..., :3].astype(np.float64)
        res = {"nonfinite_pixels_ref": int((~np.isfinite(ref).all(-1)).sum())}
        for spp in (16, 64, 256):
            r.reset()
            r.render_spp(spp, prt.seed_pairs(nf(spp)))
            img = r.read_framebuffer()[..., :3].astype(np.float64)
            res["spp%d_rmse_silhouette" % spp] = rmse(img, ref, sil)
            res["spp%d_rmse_other" % spp] = rmse(img, ref, ~sil)
            res["spp%d_nonfinite_pixels" % spp] = int((~np.isfinite(img).all(-1)).sum())
        r.reset()
        r.render_adaptive(prt.seed_pairs(nf(256)), 16, 256, 0.05)
        n = r.read_state()["samples"].reshape(H, W).astype(np.float64)
        img = r.read_framebuffer()[..., :3].astype(np.float64)
        res["adaptive"] = {"mean_paths_silhouette": round(float(n[sil].mean()), 2), "mean_paths_other": round(float(n[~sil].mean()), 2),
                           "rmse_silhouette": rmse(img, ref, sil), "rmse_other": rmse(img, ref, ~sil)}
        res["variant"] = r.kernel_variant()
        out[kind] = res
        print(json.dumps({kind: res}), file=sys.stderr, flush=True)
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--edge-scene", default="cornell_open.json")
    ap.add_argument("--edge-width", type=int, default=480)
    ap.add_argument("--edge-height", type=int, default=270)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
    prt.check_build_id()
    doc = {"tool": "tools/filter_rate.py", "build_id": prt.build_id(),
           "throughput": {"workload": "scenes/cornell_diffuse %dx%d %d spp (bench.py's headline)" % (a.width, a.height, a.spp),
                          "kinds": throughput(prt, a.width, a.height, a.spp, a.steps)}}
    print(json.dumps({"throughput": doc["throughput"]}), file=sys.stderr, flush=True)
    doc["edges"] = {"workload": "scenes/%s under the sky map, %dx%d, reference %d spp of the same filter; silhouette = unfiltered guide coverage at "
                                "K = 16 strictly between 0 and 1" % (a.edge_scene, a.edge_width, a.edge_height, a.ref_spp),
                    "results": edges(prt, a.edge_scene, a.edge_width, a.edge_height, a.ref_spp)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
