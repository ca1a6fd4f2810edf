#!/usr/bin/env python3
"""Rays per second of the ray queries (prt_cast_rays_device, prt_occluded_device) on the MI355X, and the yardstick next to them.

Per scene (cornell_diffuse and the 871 k-triangle stand-in of BASELINE config 5), on device buffers, two sets of 1920 x 1080 rays:
  primary     the pixel-centre rays of the pinhole default camera (what prt_cast_pixels generates)
  random      as many rays from uniform points in the root box of the tree, uniform unit directions, tmax = 20
each through the closest-hit and the occlusion kernel, timed with HIP events on the stream the context runs on (prt_set_stream: torch's),
around the call: the median of --calls calls.  The yardstick for the primary set is prt_render_guides(1) on the same context, timed the same
way: it walks the same rays with the same steps and moves 32 bytes per pixel against the 80 of a cast.  The event pair also covers the
launch and the call's own synchronisation (the same for both).
Both shapes of the walk loop (csrc/hip/pt_cast.hip): the library as built ("scheduled") and, with --plain-lib, a variant built with
-DPT_CAST_PLAIN_LOOP (tools/build_variant.sh plain -DPT_CAST_PLAIN_LOOP), each in a process of its own.
These are measurements to write down: there is no pass mark.  One JSON document on stdout (and into --out).

    python tools/cast_rate.py [--scenes cornell_diffuse,cornell_dragon] [--plain-lib PATH] [--out profiles/r20_cast_rays.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))          # cast_api: the ray generator and the root box, on the host

W, H = 1920, 1080


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}


def _timed(torch, fn, calls):
    out = []
    for k in range(calls + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= 2:                                               # two warm-up calls
            out.append(e0.elapsed_time(e1))
    return out


def measure(prt, name, calls):
    import torch
    import cast_api
    if "dragon" in name:
        prt.ensure_dragon_standin()
    scene = prt.HostScene(name + ".json")
    cfg = scene.config()
    cam = prt.default_camera(W, H)
    cam.apertureRadius = 0.0
    ys, xs = np.mgrid[0:H, 0:W]
    n = W * H
    primary = cast_api.pixel_rays(cam, W, H, np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32))
    box = cast_api.root_box(cfg, scene.desc).astype(np.float64)
    rng = np.random.default_rng(20)
    rnd = np.zeros((n, 8), dtype=np.float32)
    rnd[:, 0:3] = box[0::2] + rng.uniform(0, 1, (n, 3)) * (box[1::2] - box[0::2])
    d = rng.normal(size=(n, 3))
    rnd[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rnd[:, 3] = 20.0
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    r.set_camera(cam)
    r.resize(W, H)
    r.set_stream(torch.cuda.current_stream().cuda_stream)      # (main() makes a stream of torch's own current: the events and the casts share it)
    hits = torch.zeros((n, 12), dtype=torch.float32, device="cuda")
    occ = torch.zeros((n,), dtype=torch.float32, device="cuda")
    res = {"triangles": int(scene.desc.triangle_count), "rays": n}
    sys.stderr.write("cast_rate: %s loaded (%d triangles)\n" % (name, res["triangles"]))
    for label, rays in (("primary", primary), ("random", rnd)):
        d_rays = torch.from_numpy(rays).cuda()
        t_c = _timed(torch, lambda: r.cast_rays(d_rays, hits), calls)
        hit_frac = float((hits.view(torch.int32)[:, 7] != -2).float().mean().item())
        t_o = _timed(torch, lambda: r.occluded(d_rays, occ), calls)
        sys.stderr.write("cast_rate: %s, %s rays: closest %.4f ms, occluded %.4f ms\n" % (name, label, np.median(t_c), np.median(t_o)))
        res[label] = {"closest": dict(_stats(t_c), rays_per_s=round(n / (np.median(t_c) * 1e-3), 0)),
                      "occluded": dict(_stats(t_o), rays_per_s=round(n / (np.median(t_o) * 1e-3), 0)), "hit_fraction": round(hit_frac, 4)}
    t_g = _timed(torch, lambda: r.render_guides(1), calls)
    res["guides_1_sample"] = _stats(t_g)
    res["primary_closest_over_guides"] = round(float(np.median(res["primary"]["closest"]["median_ms"]) / np.median(t_g)), 3)
    r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_diffuse,cornell_dragon")
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--plain-lib", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", action="store_true", help="measure the library this process loads (PRT_LIB) and print its part")
    a = ap.parse_args()
    if a.one:
        import torch
        prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
        with torch.cuda.stream(torch.cuda.Stream()):
            print(json.dumps({"build_id": prt.build_id(), "scenes": {s: measure(prt, s, a.calls) for s in a.scenes.split(",")}}))
        return
    doc = {"what": "prt_cast_rays_device / prt_occluded_device, %d x %d rays, HIP events around the call, median of %d" % (W, H, a.calls), "loops": {}}
    for loop, lib in (("scheduled", ""), ("plain", a.plain_lib)):
        if loop == "plain" and not lib:
            continue
        env = dict(os.environ)
        if lib:
            env["PRT_LIB"] = os.path.abspath(lib)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--scenes", a.scenes, "--calls", str(a.calls)], env=env,
                             stdout=subprocess.PIPE, text=True, timeout=900)      # (the child's progress lines go to stderr as they come)
        if out.returncode != 0:
            raise SystemExit("cast_rate: the %s run failed (%d)" % (loop, out.returncode))
        doc["loops"][loop] = json.loads(out.stdout.strip().splitlines()[-1])
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
