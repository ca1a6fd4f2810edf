#!/usr/bin/env python3
"""prt_rebuild_bvh (a new Morton-order tree built on the device) against a refit and against the host's SAH builder, on the MI355X.

Per scene (the teapot of cornell_coat and the 871 k-triangle stand-in of BASELINE config 5), the mesh deformed by tools/refit_rate.py's sine
wave, every baseline timed in the same run:
  wall time, each call complete on return: prt_rebuild_bvh_device and prt_rebuild_bvh (max_leaf 4), prt_update_vertices_device, and the
      parent's rebuild path (a host load + SAH build over the deformed mesh, plus prt_upload_scene);
  bvh_cost (SAH, package helper) at 5 % and 20 % of the extent of three trees: rebuilt on the device at max_leaf 2, 4 and 8, the uploaded tree
      refitted, the host's SAH tree of the deformed mesh;
  render rate at 20 %, G segments/s of prt_render_frames (same frame, same frames, the trees taken in turn, --rounds rounds), with the
      traversal-stack levels of each tree (they size the render kernel's LDS).
Kernel times per stage: from `rocprofv3 --kernel-trace --stats` in a run of its own (this script with --phase kernels).  One JSON document on
stdout (and into --out).

    python tools/rebuild_rate.py [--scenes cornell_coat,cornell_dragon] [--out profiles/r15_rebuild.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from _trace import kernel_rows      # noqa: E402

from refit_rate import _median_ms, _scene, deform, write_mesh      # noqa: E402

KERNEL_CALLS = 5
LEAVES = (2, 4, 8)
STAGES = (("check", ("refit_check", "build_old_slot", "build_missing")), ("extent_keys", ("build_extent", "build_key")),
          ("sort_keys", None), ("nodes", ("build_node",)), ("pair_keys", ("build_pair_key",)), ("number_pairs", ("build_number", "build_pair_kernel", "build_root_slot")),
          ("records", ("refit_tri",)), ("boxes", ("refit_level", "refit_root_leaf")), ("carry", ("build_carry",)))


def stack_levels(nodes):
    """most pairs with two inner children on a path from the root, + 1 (what prt_upload_scene sizes the traversal stack by)"""
    leaf, first = nodes["leaf"] != 0, nodes["first"].astype(np.int64)
    if leaf[0]:
        return 1
    best, todo = 0, [(0, 0)]
    while todo:
        n, sp = todo.pop()
        kids = [k for k in (first[n], first[n] + 1) if not leaf[k]]
        sp += 1 if len(kids) == 2 else 0
        best = max(best, sp)
        todo += [(k, sp) for k in kids]
    return best + 1


def measure(prt, name, calls, rounds, width, height, frames):
    import torch
    scene = _scene(prt, name)
    a = prt.scene_arrays(scene.desc)
    v0, n0, nodes0 = a["vertices"].copy(), a["normals"].copy(), a["nodes"].copy()
    mesh_file = os.path.splitext(os.path.basename(scene.lib.prth_scene_obj_path(scene.handle).decode()))[0] + ".prtmesh"
    cfg = scene.config()
    out = {"triangles": int(scene.desc.triangle_count), "cost_original": prt.bvh_cost(nodes0), "stack_levels_original": stack_levels(nodes0)}
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    v20 = deform(v0, 0.20)
    dv, dn = torch.from_numpy(v20).cuda(), torch.from_numpy(n0).cuda()
    torch.cuda.synchronize()
    r.update_vertices(dv, dn)
    out["update_device_ms_median_min"] = _median_ms(lambda: r.update_vertices(dv, dn), calls)
    r.rebuild_bvh(dv, dn, 4)                                               # (the first rebuilds allocate the scratch and both sets of buffers)
    r.rebuild_bvh(dv, dn, 4)
    out["rebuild_device_ms_median_min"] = _median_ms(lambda: r.rebuild_bvh(dv, dn, 4), calls)
    out["rebuild_device_no_normals_ms_median_min"] = _median_ms(lambda: r.rebuild_bvh(dv, None, 4), calls)
    out["rebuild_host_ms_median_min"] = _median_ms(lambda: r.rebuild_bvh(v20, n0, 4), max(calls // 2, 3))
    out["rebuild_device_by_leaf_ms_median"] = {str(ml): _median_ms(lambda: r.rebuild_bvh(dv, dn, ml), max(calls // 2, 3))[0] for ml in (1,) + LEAVES + (16,)}

    # costs: rebuilt, refitted, host SAH; the trees of the 20 % mesh are kept for the render rate
    trees, out["deformations"] = {}, {}
    with tempfile.TemporaryDirectory() as d:
        for amount in (0.05, 0.20):
            v = deform(v0, amount)
            rec = {}
            for ml in LEAVES:
                r.rebuild_bvh(v, n0, ml)
                nodes, prims = r.read_bvh()
                rec["rebuilt_leaf_%d" % ml] = {"bvh_cost": prt.bvh_cost(nodes), "pairs": (len(nodes) - 1) // 2, "stack_levels": stack_levels(nodes)}
            write_mesh(os.path.join(d, mesh_file), v, n0)
            t = time.perf_counter()
            host = prt.HostScene(name + ".json", models_dir=d)
            build_s = time.perf_counter() - t
            t = time.perf_counter()
            r.upload_scene(host)
            r.synchronize()
            upload_s = time.perf_counter() - t
            hn = prt.scene_arrays(host.desc)["nodes"]
            rec["host_sah"] = {"bvh_cost": prt.bvh_cost(hn), "pairs": int((hn["leaf"] == 0).sum()), "stack_levels": stack_levels(hn),
                               "load_and_build_ms": round(1e3 * build_s, 2), "upload_scene_ms": round(1e3 * upload_s, 2),
                               "total_ms": round(1e3 * (build_s + upload_s), 2)}
            r.upload_scene(scene)
            r.update_vertices(v, None)
            rec["refitted"] = {"bvh_cost": prt.bvh_cost(nodes0, r.read_bvh_bounds()), "pairs": int((nodes0["leaf"] == 0).sum()),
                               "stack_levels": stack_levels(nodes0)}
            for k in rec:
                rec[k]["over_host_sah"] = round(rec[k]["bvh_cost"] / rec["host_sah"]["bvh_cost"], 4)
            out["deformations"]["%g" % amount] = rec
            if amount == 0.20:
                trees["host_sah"] = host
            else:
                host.close()
        # render rate at 20 %: one context per tree, taken in turn
        cam, seeds = prt.default_camera(width, height), prt.seed_pairs(frames)
        ctx = {}
        for arm in ["refitted", "host_sah"] + ["rebuilt_leaf_%d" % ml for ml in LEAVES]:
            q = prt.Renderer(cfg, device=0)
            q.upload_scene(trees["host_sah"] if arm == "host_sah" else scene)
            if arm == "refitted":
                q.update_vertices(v20, n0)
            elif arm != "host_sah":
                q.rebuild_bvh(v20, n0, int(arm.rsplit("_", 1)[1]))
            q.set_camera(cam)
            q.resize(width, height)
            ctx[arm] = q
        rate = {arm: [] for arm in ctx}
        for k in range(rounds + 1):
            for arm in (list(ctx) if k % 2 == 0 else list(ctx)[::-1]):
                q = ctx[arm]
                q.reset()
                q.synchronize()
                t = time.perf_counter()
                q.render_frames(seeds)
                q.synchronize()
                dt = time.perf_counter() - t
                if k:                                                      # (round 0 warms up)
                    rate[arm].append(width * height * frames / dt / 1e9)
        out["render_rate_20"] = {"frame": [width, height], "frames": frames, "rounds": rounds,
                                 "gsegments_per_s": {arm: {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4),
                                                           "max": round(float(max(v)), 4), "variant": ctx[arm].kernel_variant(),
                                                           "stack_levels": out["deformations"]["0.2"][arm]["stack_levels"]} for arm, v in rate.items()}}
        for q in ctx.values():
            q.close()
        trees["host_sah"].close()
    r.close()
    return out


def kernels_phase(prt, names):
    """the launches rocprofv3 times: KERNEL_CALLS device rebuilds (with normals, motion off, max_leaf 4) per scene"""
    import torch
    for name in names:
        scene = _scene(prt, name)
        a = prt.scene_arrays(scene.desc)
        r = prt.Renderer(scene.config(), device=0)
        r.upload_scene(scene)
        dv, dn = torch.from_numpy(deform(a["vertices"], 0.20)).cuda(), torch.from_numpy(a["normals"].copy()).cuda()
        torch.cuda.synchronize()
        for _ in range(KERNEL_CALLS):
            r.rebuild_bvh(dv, dn, 4)
        r.close()


def kernel_times(names, timeout):
    rows = kernel_rows(["--phase", "kernels", "--scenes", ",".join(names)], "rebuild", timeout)
    # one rebuild = a check launch and everything up to the next one
    starts = [i for i, r in enumerate(rows) if "refit_check" in r[0]]
    assert len(starts) == KERNEL_CALLS * len(names), (len(starts), len(rows))
    out = {}
    for s, name in enumerate(names):
        best = None
        for c in range(2, KERNEL_CALLS):                     # (calls 0 and 1 allocate)
            i = starts[s * KERNEL_CALLS + c]
            j = starts[s * KERNEL_CALLS + c + 1] if s * KERNEL_CALLS + c + 1 < len(starts) else len(rows)
            one = rows[i:j]
            own = [pat for _, pats in STAGES if pats for pat in pats]
            rec = {}
            for stage, pats in STAGES:
                # the library's kernels (the two sorts and the scan) are whatever is no kernel of the project's own
                sel = [r for r in one if (any(p in r[0] for p in pats) if pats else not any(p in r[0] for p in own))]
                rec[stage + "_us"] = round(sum(e - b for _, b, e in sel) / 1e3, 2)
                rec[stage + "_launches"] = len(sel)
            rec["busy_us"] = round(sum(e - b for _, b, e in one) / 1e3, 2)
            rec["span_us"] = round((one[-1][2] - one[0][1]) / 1e3, 2)
            if best is None or rec["span_us"] < best["span_us"]:
                best = rec
        out[name] = best
    out["note"] = "kernel durations of one prt_rebuild_bvh_device call (best of %d), rocprofv3 --kernel-trace --stats; sort_keys = every kernel " \
                  "that is not the project's own (both radix sorts and the scan); span = the first kernel's start to the last one's end, the two " \
                  "host round trips included" % (KERNEL_CALLS - 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_coat,cornell_dragon")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--phase", default="all", choices=["all", "rates", "kernels"])
    ap.add_argument("--rocprof-timeout", type=int, default=300)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
    names = a.scenes.split(",")
    if a.phase == "kernels":
        kernels_phase(prt, names)
        return
    w, h = (int(x) for x in a.size.split("x"))
    doc = {"build_id": prt.build_id(), "calls": a.calls, "scenes": {}}
    for name in names:
        doc["scenes"][name] = measure(prt, name, a.calls, a.rounds, w, h, a.frames)
        print(json.dumps({name: doc["scenes"][name]}), file=sys.stderr, flush=True)
    if a.phase == "all":
        try:
            doc["kernel_time"] = kernel_times(names, a.rocprof_timeout)
        except (subprocess.SubprocessError, AssertionError, KeyError, OSError) as e:
            doc["kernel_time"] = {"error": repr(e)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
