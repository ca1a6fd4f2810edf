#!/usr/bin/env python3
"""prt_bvh_cost and prt_set_rebuild_policy (the tree's cost and the rebuild rule on the device) against what they replace, on the MI355X.

Per scene (the 871 k-triangle stand-in of BASELINE config 5 by default), all in one run, wall clock, each call complete on return:
  bvh_cost_device     prt_bvh_cost: the launches and 8 bytes back
  read_back_and_host  the parent's path: prt_read_bvh (36 bytes per node) plus the numpy bvh_cost over the nodes
  update_policy_off   prt_update_vertices_device from device buffers
  update_policy_on    the same call with a policy whose limit is never reached: what the cost check adds to every refit
                      (the two arms on two contexts of the same scene, alternated call by call, medians over --calls rounds)
and an animation: the sine deformations of tools/refit_rate.py at 1, 5 and 20 % of the extent, two frames each at different phases, through
three contexts -- the policy at --limit (1.3), refit only (no policy), rebuild every frame -- with, per frame: the time of the geometry
call, the cost, whether the policy rebuilt, and the render rate (G segments/s of prt_render_frames, same frame and frames, the contexts
taken in turn).  The figures are reported as measured; there is no pass mark.  One JSON document on stdout (and into --out).

    python tools/bvh_cost_rate.py [--scenes cornell_dragon] [--out profiles/r24_bvh_cost.json]
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
from refit_rate import _median_ms, _scene, deform      # noqa: E402


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}


def measure(prt, name, calls, limit, max_leaf, width, height, frames):
    import torch
    scene = _scene(prt, name)
    a = prt.scene_arrays(scene.desc)
    v0, n0 = a["vertices"].copy(), a["normals"].copy()
    cfg = scene.config()
    out = {"triangles": int(scene.desc.triangle_count), "bvh_nodes": int(scene.desc.bvh_node_count), "limit": limit, "max_leaf": max_leaf}
    dn = torch.from_numpy(n0).cuda()
    dv = [torch.from_numpy(deform(v0, 0.01, phase=0.05 * k)).cuda() for k in range(2)]
    torch.cuda.synchronize()

    # the cost call against the read-back and the host loop
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    r.update_vertices(dv[0], dn)
    cost = r.bvh_cost()                                                    # (the first call allocates the partial sums)
    out["bvh_cost_device_ms_median_min"] = _median_ms(r.bvh_cost, calls)
    host = {"read_bvh": [], "numpy_bvh_cost": []}
    for _ in range(max(calls // 4, 3)):
        t = time.perf_counter()
        nodes, _prims = r.read_bvh()
        t1 = time.perf_counter()
        host_cost = prt.bvh_cost(nodes)
        host["read_bvh"].append(1e3 * (t1 - t))
        host["numpy_bvh_cost"].append(1e3 * (time.perf_counter() - t1))
    out["read_back_and_host"] = {k: _stats(v) for k, v in host.items()}
    out["read_back_and_host"]["total_median_ms"] = round(sum(x["median_ms"] for x in out["read_back_and_host"].values()), 4)
    out["read_back_and_host"]["bytes_read"] = 36 * len(nodes) + 8 * int(scene.desc.triangle_count)
    out["cost"] = {"device": cost, "host": host_cost, "relative_difference": abs(cost - host_cost) / host_cost}
    out["read_back_and_host_over_device"] = round(out["read_back_and_host"]["total_median_ms"] / out["bvh_cost_device_ms_median_min"][0], 1)

    # what the check adds to a refit that does not rebuild: two contexts, alternated
    q = prt.Renderer(cfg, device=0)
    q.upload_scene(scene)
    q.update_vertices(dv[0], dn)
    q.set_rebuild_policy(1e30, max_leaf)
    arms = {"off": r, "on": q}
    t = {arm: [] for arm in arms}
    for k in range(calls + 2):
        for arm in (("off", "on") if k % 2 == 0 else ("on", "off")):
            t0 = time.perf_counter()
            arms[arm].update_vertices(dv[k % 2], dn)
            if k >= 2:
                t[arm].append(1e3 * (time.perf_counter() - t0))
    out["update_policy_off"], out["update_policy_on"] = _stats(t["off"]), _stats(t["on"])
    out["policy_on_minus_off_median_ms"] = round(out["update_policy_on"]["median_ms"] - out["update_policy_off"]["median_ms"], 4)
    out["policy_on_over_off_median"] = round(out["update_policy_on"]["median_ms"] / out["update_policy_off"]["median_ms"], 3)
    assert q.rebuild_report()["rebuilds"] == 0
    r.close()
    q.close()

    # the animation
    cam, seeds = prt.default_camera(width, height), prt.seed_pairs(frames)
    ctx = {}
    for arm in ("policy", "refit_only", "rebuild_every_frame"):
        c = prt.Renderer(cfg, device=0)
        c.upload_scene(scene)
        c.set_camera(cam)
        c.resize(width, height)
        if arm == "rebuild_every_frame":
            c.rebuild_bvh(dv[0], dn, max_leaf)                             # (the first rebuild allocates the scratch and the spare set)
        c.update_vertices(torch.from_numpy(v0).cuda(), dn)                 # (the first update uploads the tables)
        if arm == "policy":
            c.set_rebuild_policy(limit, max_leaf)
        c.reset()
        c.render_frames(seeds)                                             # (warm-up: code objects, first launches)
        ctx[arm] = c
    out["animation"] = {"frame": [width, height], "frames_per_render": frames, "steps": []}
    step = 0
    for amount in (0.01, 0.05, 0.20):
        for phase in (0.0, 0.13):
            d = torch.from_numpy(deform(v0, amount, phase=phase)).cuda()
            torch.cuda.synchronize()
            rec = {"deformation": amount, "phase": phase}
            for arm in (list(ctx) if step % 2 == 0 else list(ctx)[::-1]):
                c = ctx[arm]
                t0 = time.perf_counter()
                if arm == "rebuild_every_frame":
                    c.rebuild_bvh(d, dn, max_leaf)
                else:
                    c.update_vertices(d, dn)
                geometry_ms = 1e3 * (time.perf_counter() - t0)
                c.reset()
                c.synchronize()
                t0 = time.perf_counter()
                c.render_frames(seeds)
                c.synchronize()
                dt = time.perf_counter() - t0
                rec[arm] = {"geometry_ms": round(geometry_ms, 4), "bvh_cost": c.bvh_cost(), "gsegments_per_s": round(width * height * frames / dt / 1e9, 4)}
                if arm == "policy":
                    rep = c.rebuild_report()
                    rec[arm].update(rebuilt=rep["rebuilt"], baseline=rep["baseline"], cost_after_refit=rep["cost"])
            out["animation"]["steps"].append(rec)
            step += 1
    out["animation"]["policy_rebuilds"] = ctx["policy"].rebuild_report()["rebuilds"]
    for arm in ctx:
        rates = [s[arm]["gsegments_per_s"] for s in out["animation"]["steps"]]
        out["animation"][arm + "_gsegments_per_s_mean"] = round(float(np.mean(rates)), 4)
        out["animation"][arm + "_geometry_ms_mean"] = round(float(np.mean([s[arm]["geometry_ms"] for s in out["animation"]["steps"]])), 4)
    for c in ctx.values():
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_dragon")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--limit", type=float, default=1.3)
    ap.add_argument("--max-leaf", type=int, default=4)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
    doc = {"build_id": prt.build_id(), "calls": a.calls, "scenes": {}}
    for name in a.scenes.split(","):
        doc["scenes"][name] = measure(prt, name, a.calls, a.limit, a.max_leaf, a.width, a.height, a.frames)
        print(json.dumps({name: doc["scenes"][name]}), file=sys.stderr, flush=True)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
