#!/usr/bin/env python3
"""prt_update_vertices (the device refit of a deforming mesh) against what the same change cost before it existed, on the MI355X.

Per scene (the teapot of cornell_coat and the 871 k-triangle stand-in of BASELINE config 5): the mesh is deformed by a sine wave of 1, 5 and
20 % of its extent (float32 numpy), and timed, wall clock, each call complete on return:
  update_device      prt_update_vertices_device from device buffers (vertices + normals)
  update_host        prt_update_vertices from host arrays (PCIe included)
  rebuild_upload     the parent's path: a host build over the deformed mesh (HostScene on a mesh file written for it: reading the file, the
                     SAH build) plus prt_upload_scene
  refit_upload       the parent's cheaper path: the caller's nodes refitted in numpy (vectorised, by value) plus prt_upload_scene alone
and bvh_cost (SAH, package helper) of the refitted tree against the rebuilt one per deformation.
With --phase motion (prt_set_motion): what the motion mode adds, two contexts (motion on / off) timed alternately, call by call, medians over
--calls rounds: an update with and without the snapshot copy (a small guide render between the timed calls consumes the snapshot, so every
timed update of the "on" arm takes one), prt_render_guides (4 samples) at 1920x1080 with the motion instance and with the plain one, and
prt_denoise_temporal with and without the plane.
With --phase normals (prt_set_smooth_normals): an update of the scene's mesh from device buffers with GENERATED normals (normals NULL, the
topology set; unit and area weighting) against the same update with the caller's device normals -- the existing path, the baseline --, the
arms alternated call by call on contexts of the same scene, medians over --calls rounds, each call complete on return; and the kernels of one
generated update from a rocprofv3 run of its own (--phase normals-kernels).  Both times and their ratio are reported; there is no pass mark.
Kernel times: from `rocprofv3 --kernel-trace --stats` in a run of its own (this script with --phase kernels).  One JSON document on stdout
(and into --out).

    python tools/refit_rate.py [--scenes cornell_coat,cornell_dragon] [--out profiles/r12_refit.json]
"""
import argparse
import importlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _trace import kernel_rows      # noqa: E402

KERNEL_CALLS = 5
f32 = np.float32


def deform(v0, amount, phase=0.0):
    """a sine wave across y that pushes x and z by `amount` x the mesh's largest extent"""
    v = v0.copy()
    lo, hi = v0[:, :3].min(axis=0), v0[:, :3].max(axis=0)
    ext = f32((hi - lo).max())
    t = ((v0[:, 1] - lo[1]) / f32(max(hi[1] - lo[1], 1e-6))).astype(f32)
    w = np.sin(f32(6.2831853) * (f32(3.0) * t + f32(phase))).astype(f32)
    v[:, 0] += f32(amount) * ext * w
    v[:, 2] += f32(amount) * ext * np.cos(f32(6.2831853) * (f32(2.0) * t + f32(phase))).astype(f32)
    return v


def numpy_refit(nodes, pi, v):
    """the caller's nodes refitted in numpy, vectorised: leaf boxes by reduceat over the leaves' vertices, inner boxes level by level from
    the deepest (by value: np.minimum does not pin the sign of a zero, which a timing baseline does not need)"""
    out = nodes.copy()
    leaf = nodes["leaf"] != 0
    first, count = nodes["first"].astype(np.int64), nodes["count"].astype(np.int64)
    levels, front = [], np.array([0], dtype=np.int64)
    while front.size:
        levels.append(front)
        inner = front[~leaf[front]]
        nxt = np.concatenate([first[inner], first[inner] + 1])
        front = nxt
    lv = np.nonzero(leaf & (count > 0))[0]
    if lv.size:
        starts = np.concatenate([[0], np.cumsum(count[lv])[:-1]])
        which = np.repeat(np.arange(lv.size), count[lv])
        tri = pi[(first[lv][which] + (np.arange(which.size) - starts[which]))].astype(np.int64)
        pts = v[(3 * tri[:, None] + np.arange(3)[None, :]).reshape(-1), :3]
        b = out["bounds"]
        b[lv, 0::2] = np.minimum.reduceat(pts, 3 * starts, axis=0)
        b[lv, 1::2] = np.maximum.reduceat(pts, 3 * starts, axis=0)
    for members in reversed(levels):
        inner = members[~leaf[members]]
        b = out["bounds"]
        b[inner, 0::2] = np.minimum(b[first[inner], 0::2], b[first[inner] + 1, 0::2])
        b[inner, 1::2] = np.maximum(b[first[inner], 1::2], b[first[inner] + 1, 1::2])
    return out


def write_mesh(path, v, n):
    tris = np.concatenate([v[:, :3], n[:, :3]], axis=1).astype(f32).reshape(-1, 3, 6)
    with open(path, "wb") as fh:
        fh.write(b"PRTMESH1")
        fh.write(struct.pack("<I", tris.shape[0]))
        fh.write(tris.tobytes())


def _scene(prt, name):
    if "dragon" in name:
        prt.ensure_dragon_standin()
    return prt.HostScene(name + ".json")


def _median_ms(fn, n):
    out = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t))
    return round(float(np.median(out)), 4), round(float(min(out)), 4)


def measure(prt, name, calls):
    import ctypes as C
    import torch
    scene = _scene(prt, name)
    a = prt.scene_arrays(scene.desc)
    v0, n0, pi, nodes = a["vertices"].copy(), a["normals"].copy(), a["primitive_indices"].copy(), a["nodes"].copy()
    mesh_file = os.path.splitext(os.path.basename(scene.lib.prth_scene_obj_path(scene.handle).decode()))[0] + ".prtmesh"   # (the loader falls back to it)
    cfg = scene.config()
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    out = {"triangles": int(scene.desc.triangle_count), "bvh_nodes": int(scene.desc.bvh_node_count), "cost_original": prt.bvh_cost(nodes)}
    assert (r.read_bvh_bounds() == nodes["bounds"]).all()
    v1 = deform(v0, 0.01)
    dv, dn = torch.from_numpy(v1).cuda(), torch.from_numpy(n0).cuda()
    torch.cuda.synchronize()
    r.update_vertices(dv, dn)                                              # (the first update uploads the tables)
    out["update_device_ms_median_min"] = _median_ms(lambda: r.update_vertices(dv, dn), calls)
    out["update_device_no_normals_ms_median_min"] = _median_ms(lambda: r.update_vertices(dv, None), calls)
    out["update_host_ms_median_min"] = _median_ms(lambda: r.update_vertices(v1, n0), max(calls // 2, 3))
    assert (r.read_bvh_bounds() == numpy_refit(nodes, pi, v1)["bounds"]).all(), "the device refit disagrees with the numpy refit"

    # the parent's paths for the same change
    t = time.perf_counter()
    nodes1 = numpy_refit(nodes, pi, v1)
    numpy_s = time.perf_counter() - t
    desc = prt.SceneDesc.from_buffer_copy(bytes(scene.desc))
    desc.vertices, desc.normals = v1.ctypes.data_as(C.c_void_p), n0.ctypes.data_as(C.c_void_p)
    desc.bvh_nodes = nodes1.ctypes.data_as(C.c_void_p)

    def upload():
        r.upload_scene(desc)
        r.synchronize()
    up = _median_ms(upload, 3)
    out["refit_upload"] = {"numpy_refit_ms": round(1e3 * numpy_s, 2), "upload_scene_ms_median_min": up, "total_ms": round(1e3 * numpy_s + up[0], 2)}
    out["deformations"] = {}
    with tempfile.TemporaryDirectory() as d:
        for amount in (0.01, 0.05, 0.20):
            v = deform(v0, amount)
            write_mesh(os.path.join(d, mesh_file), v, n0)
            t = time.perf_counter()
            rebuilt = prt.HostScene(name + ".json", models_dir=d)
            build_s = time.perf_counter() - t
            t = time.perf_counter()
            r.upload_scene(rebuilt)
            r.synchronize()
            upload_s = time.perf_counter() - t
            cost_rebuilt = prt.bvh_cost(prt.scene_arrays(rebuilt.desc)["nodes"])
            r.upload_scene(scene)                                          # back to the original tree, refitted to the same vertices
            r.update_vertices(v, None)
            cost_refit = prt.bvh_cost(nodes, r.read_bvh_bounds())
            out["deformations"]["%g" % amount] = {
                "rebuild_upload": {"load_and_build_ms": round(1e3 * build_s, 2), "upload_scene_ms": round(1e3 * upload_s, 2),
                                   "total_ms": round(1e3 * (build_s + upload_s), 2)},
                "bvh_cost_refitted": cost_refit, "bvh_cost_rebuilt": cost_rebuilt, "refitted_over_rebuilt": round(cost_refit / cost_rebuilt, 4)}
            rebuilt.close()
    dev = out["update_device_ms_median_min"][0]
    out["ratio_to_parent"] = {"rebuild_upload_over_update_device": round(out["deformations"]["0.01"]["rebuild_upload"]["total_ms"] / dev, 1),
                              "refit_upload_over_update_device": round(out["refit_upload"]["total_ms"] / dev, 1),
                              "rebuild_upload_over_update_host": round(out["deformations"]["0.01"]["rebuild_upload"]["total_ms"] / out["update_host_ms_median_min"][0], 1)}
    r.close()
    return out


def motion_phase(prt, name, rounds, width=1920, height=1080):
    """the cost of prt_set_motion on scene `name`: {update, guides, temporal} x {off, on}, arms alternated within every round"""
    import torch
    scene = _scene(prt, name)
    a = prt.scene_arrays(scene.desc)
    v0, n0 = a["vertices"].copy(), a["normals"].copy()
    cfg = scene.config()
    cam = prt.default_camera(width, height)
    dn = torch.from_numpy(n0).cuda()
    dv = [torch.from_numpy(deform(v0, 0.01, phase=0.05 * k)).cuda() for k in range(2)]
    torch.cuda.synchronize()
    arms = {}
    for arm in ("off", "on"):
        small, big = prt.Renderer(cfg, device=0), prt.Renderer(cfg, device=0)
        for r, (w, h) in ((small, (64, 48)), (big, (width, height))):
            r.upload_scene(scene)
            r.set_camera(prt.default_camera(w, h))
            r.resize(w, h)
            r.set_motion(arm == "on")
            r.update_vertices(dv[0], dn)                                   # (the first update uploads the tables and allocates the snapshot)
            r.render_guides(1)
        big.reset()
        big.render_spp(1, prt.seed_pairs(4 * max(cfg.max_bounces, 8) + 64))
        arms[arm] = (small, big)
    t = {k: {"off": [], "on": []} for k in ("update", "guides", "temporal")}

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)
    for k in range(rounds + 2):
        for arm in (("off", "on") if k % 2 == 0 else ("on", "off")):
            small, big = arms[arm]
            small.render_guides(1)                                         # consumes a pending snapshot: the timed update takes a fresh one
            ms_u = timed(lambda: small.update_vertices(dv[k % 2], dn))
            big.update_vertices(dv[k % 2], dn)
            ms_g = timed(lambda: big.render_guides(4))
            ms_t = timed(lambda: big.denoise_temporal())
            if k >= 2:                                                     # (two warm-up rounds: allocations, first launches)
                t["update"][arm].append(ms_u); t["guides"][arm].append(ms_g); t["temporal"][arm].append(ms_t)
    moving = float((np.abs(arms["on"][1].read_motion()[..., :3]).max(-1) > 0).mean())
    for small, big in arms.values():
        small.close()
        big.close()
    out = {"triangles": int(scene.desc.triangle_count), "frame": [width, height], "rounds": rounds, "guide_samples": 4,
           "pixels_with_motion": round(moving, 4), "snapshot_bytes": 48 * int(scene.desc.triangle_count)}
    for k, arms_t in t.items():
        out[k] = {arm: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}
                  for arm, v in arms_t.items()}
        out[k]["on_minus_off_median_ms"] = round(out[k]["on"]["median_ms"] - out[k]["off"]["median_ms"], 4)
    return out


def normals_phase(prt, name, rounds):
    """the cost of generated normals on scene `name`: update_vertices from device buffers, {caller's normals, generated unit, generated area}"""
    import torch
    scene = _scene(prt, name)
    a = prt.scene_arrays(scene.desc)
    v0, n0 = a["vertices"].copy(), a["normals"].copy()
    t0 = time.perf_counter()
    groups, n_groups = prt.weld_corners(v0)
    weld_ms = 1e3 * (time.perf_counter() - t0)
    valence = np.bincount(groups)
    cfg = scene.config()
    dn = torch.from_numpy(n0).cuda()
    dv = [torch.from_numpy(deform(v0, 0.01, phase=0.05 * k)).cuda() for k in range(2)]
    torch.cuda.synchronize()
    ctx, set_ms = {}, {}
    for arm in ("unit", "area"):
        r = prt.Renderer(cfg, device=0)
        r.upload_scene(scene)
        t0 = time.perf_counter()
        r.set_smooth_normals(groups, n_groups, arm)
        set_ms[arm] = round(1e3 * (time.perf_counter() - t0), 3)
        ctx[arm] = r
    arms = {"explicit": (ctx["unit"], dn), "generated_unit": (ctx["unit"], None), "generated_area": (ctx["area"], None)}
    for r, n in arms.values():                                             # (the first update uploads the tables; first launches load code)
        for k in range(2):
            r.update_vertices(dv[k], n)
    t = {arm: [] for arm in arms}
    names = list(arms)
    for k in range(rounds):
        for arm in names[k % 3:] + names[:k % 3]:                          # (the arms alternate, the order rotates)
            r, n = arms[arm]
            t0 = time.perf_counter()
            r.update_vertices(dv[k % 2], n)
            t[arm].append(1e3 * (time.perf_counter() - t0))
    ctx["unit"].update_vertices(dv[0], None)
    gen = ctx["unit"].read_normals()
    ctx["unit"].update_vertices(dv[0], None)
    same = bool(np.array_equal(gen.view(np.uint32), ctx["unit"].read_normals().view(np.uint32)))      # (the same call again: the same bits)
    for r in ctx.values():
        r.close()
    out = {"triangles": int(scene.desc.triangle_count), "groups": int(n_groups), "rounds": rounds,
           "valence": {"min": int(valence.min()), "median": float(np.median(valence)), "max": int(valence.max()),
                       "sum_of_squares": int((valence.astype(np.int64) ** 2).sum())},
           "weld_corners_host_ms": round(weld_ms, 2), "set_smooth_normals_ms": set_ms,
           "device_bytes": {"unit": 88 * int(scene.desc.triangle_count) + 4 * (n_groups + 1), "area": 104 * int(scene.desc.triangle_count) + 4 * (n_groups + 1)},
           "generated_normals_unit_length": bool(np.abs(np.linalg.norm(gen[:, :3].astype(np.float64), axis=1) - 1).max() < 1e-5), "stable": same}
    for arm, v in t.items():
        out[arm] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}
    for arm in ("generated_unit", "generated_area"):
        out[arm]["over_explicit_median"] = round(out[arm]["median_ms"] / out["explicit"]["median_ms"], 3)
        out[arm]["minus_explicit_median_ms"] = round(out[arm]["median_ms"] - out["explicit"]["median_ms"], 4)
    return out


def normals_kernels_phase(prt, names):
    """the launches rocprofv3 times: KERNEL_CALLS device updates with generated normals (unit weighting) per scene"""
    import torch
    for name in names:
        scene = _scene(prt, name)
        a = prt.scene_arrays(scene.desc)
        r = prt.Renderer(scene.config(), device=0)
        r.upload_scene(scene)
        r.set_smooth_normals(*prt.weld_corners(a["vertices"]))
        dv = torch.from_numpy(deform(a["vertices"], 0.01)).cuda()
        torch.cuda.synchronize()
        for _ in range(KERNEL_CALLS):
            r.update_vertices(dv, None)
        r.close()


def normals_kernel_times(names, timeout):
    """per scene: the durations of the kernels of one generated update (best of the calls after the first), by kernel"""
    rows = [r for r in kernel_rows(["--phase", "normals-kernels", "--scenes", ",".join(names)], "normals", timeout) if "refit_" in r[0] or "normals_" in r[0]]
    starts = [i for i, r in enumerate(rows) if "refit_check" in r[0]]
    assert len(starts) == KERNEL_CALLS * len(names), (len(starts), len(rows))
    out = {}
    for s, name in enumerate(names):
        best = None
        for c in range(1, KERNEL_CALLS):
            i = starts[s * KERNEL_CALLS + c]
            j = starts[s * KERNEL_CALLS + c + 1] if s * KERNEL_CALLS + c + 1 < len(starts) else len(rows)
            one = rows[i:j]
            us = lambda key: round(sum(e - b for n, b, e in one if key in n) / 1e3, 2)
            rec = {"check_us": us("refit_check"), "normals_face_us": us("normals_face"), "normals_corner_us": us("normals_corner"),
                   "refit_tri_us": us("refit_tri"), "refit_levels_busy_us": round(us("refit_level") + us("refit_root_leaf"), 2),
                   "face_to_root_span_us": round((one[-1][2] - one[1][1]) / 1e3, 2) if len(one) > 1 else 0.0}
            if best is None or rec["face_to_root_span_us"] < best["face_to_root_span_us"]:
                best = rec
        out[name] = best
    out["note"] = "kernel durations of one prt_update_vertices_device call with generated normals (best of %d), rocprofv3 --kernel-trace --stats" % (KERNEL_CALLS - 1)
    return out


def kernels_phase(prt, names):
    """the launches rocprofv3 times: KERNEL_CALLS device updates (with normals) per scene"""
    import torch
    for name in names:
        scene = _scene(prt, name)
        a = prt.scene_arrays(scene.desc)
        r = prt.Renderer(scene.config(), device=0)
        r.upload_scene(scene)
        dv, dn = torch.from_numpy(deform(a["vertices"], 0.05)).cuda(), torch.from_numpy(a["normals"].copy()).cuda()
        torch.cuda.synchronize()
        for _ in range(KERNEL_CALLS):
            r.update_vertices(dv, dn)
        r.close()


def kernel_times(names, timeout):
    rows = [r for r in kernel_rows(["--phase", "kernels", "--scenes", ",".join(names)], "refit", timeout) if "refit_" in r[0]]
    # one update = a check launch and everything up to the next one
    starts = [i for i, r in enumerate(rows) if "refit_check" in r[0]]
    assert len(starts) == KERNEL_CALLS * len(names), (len(starts), len(rows))
    out = {}
    for s, name in enumerate(names):
        best = None
        for c in range(1, KERNEL_CALLS):                     # (call 0 follows the tables' upload)
            i = starts[s * KERNEL_CALLS + c]
            j = starts[s * KERNEL_CALLS + c + 1] if s * KERNEL_CALLS + c + 1 < len(starts) else len(rows)
            one = rows[i:j]
            lv = [r for r in one if "refit_level" in r[0] or "refit_root_leaf" in r[0]]
            rec = {"check_us": round(sum(e - b for n, b, e in one if "refit_check" in n) / 1e3, 2),
                   "tri_us": round(sum(e - b for n, b, e in one if "refit_tri" in n) / 1e3, 2),
                   "levels_busy_us": round(sum(e - b for n, b, e in lv) / 1e3, 2), "level_launches": len(lv),
                   "levels_span_us": round((lv[-1][2] - lv[0][1]) / 1e3, 2) if lv else 0.0,
                   "tri_to_root_span_us": round((one[-1][2] - one[1][1]) / 1e3, 2) if len(one) > 1 else 0.0}
            if best is None or rec["tri_to_root_span_us"] < best["tri_to_root_span_us"]:
                best = rec
        out[name] = best
    out["note"] = "kernel durations of one prt_update_vertices_device call (best of %d), rocprofv3 --kernel-trace --stats; levels_span = first " \
                  "level's start to the root's end (launch gaps included), levels_busy = the sum of the level kernels' own durations" % (KERNEL_CALLS - 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_coat,cornell_dragon")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--phase", default="all", choices=["all", "rates", "kernels", "motion", "normals", "normals-kernels"])
    ap.add_argument("--rocprof-timeout", type=int, default=300)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
    names = a.scenes.split(",")
    if a.phase == "kernels":
        kernels_phase(prt, names)
        return
    if a.phase == "normals-kernels":
        normals_kernels_phase(prt, names)
        return
    if a.phase == "normals":
        doc = {"build_id": prt.build_id(), "normals": {name: normals_phase(prt, name, a.calls) for name in names}}
        try:
            doc["kernel_time"] = normals_kernel_times(names, a.rocprof_timeout)
        except (subprocess.SubprocessError, AssertionError, KeyError, OSError) as e:
            doc["kernel_time"] = {"error": repr(e)}
        text = json.dumps(doc, indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(text + "\n")
        return
    if a.phase == "motion":
        doc = {"build_id": prt.build_id(), "motion": {name: motion_phase(prt, name, a.calls) for name in names}}
        text = json.dumps(doc, indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(text + "\n")
        return
    doc = {"build_id": prt.build_id(), "calls": a.calls, "scenes": {}}
    for name in names:
        doc["scenes"][name] = measure(prt, name, a.calls)
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
