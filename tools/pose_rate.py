#!/usr/bin/env python3
"""prt_pose (the mesh posed on the device from bone matrices) against the parent's routes to the same scene, on the MI355X.

Per scene (the teapot of cornell_coat and the 871 k-triangle stand-in of cornell_dragon) and per skin (rigid parts -- w = (1, 0, 0, 0) -- and
four influences per corner, with 16 and 256 bones), wall clock per call, each call complete on return, the arms of one group alternated
call by call with a rotating order, medians over --calls rounds:
  pose_host_refit / pose_device_refit        prt_pose (n_bones x 48 bytes from host memory) / prt_pose_device, PRT_POSE_REFIT
  update_device / update_host                the parent's routes: prt_update_vertices_device from device buffers holding the posed vertices
                                             and normals / prt_update_vertices from host arrays (PCIe included)
  pose_host_rebuild / pose_device_rebuild    the same two doors, PRT_POSE_REBUILD
  rebuild_device                             prt_rebuild_bvh_device from device buffers
The posed arrays the parent's routes are given are prt_read_posed's of the same skin and matrices: all arms leave the same scene.
Kernel time: pose_kernel's duration from `rocprofv3 --kernel-trace --stats` in a run of its own (this script with --phase kernels), and
its streamed bytes (88 per corner with normals: 16 + 16 + 8 + 16 in, 16 + 16 out; the matrix table is not counted) per second.  One JSON
document on stdout (and into --out).  There is no pass mark.

    python tools/pose_rate.py [--scenes cornell_coat,cornell_dragon] [--out profiles/r22_pose.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _trace import kernel_rows      # noqa: E402

KERNEL_CALLS = 5
SKINS = [("rigid", 16), ("rigid", 256), ("four", 16), ("four", 256)]
f32 = np.float32


def _scene(prt, name):
    if "dragon" in name:
        prt.ensure_dragon_standin()
    return prt.HostScene(name + ".json")


def bones(n_bones, seed):
    """small rotations about y with a small shift: float32 [n_bones, 12]"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-0.05, 0.05, n_bones)
    M = np.zeros((n_bones, 3, 4))
    M[:, 0, 0], M[:, 0, 2], M[:, 2, 0], M[:, 2, 2], M[:, 1, 1] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang), 1.0
    M[:, :, 3] = rng.uniform(-0.01, 0.01, (n_bones, 3))
    return np.ascontiguousarray(M.reshape(n_bones, 12), dtype=f32)


def influences(v0, kind, n_bones, seed):
    """bones as slabs along y: a rigid corner belongs to its triangle's slab, a four-influence corner to its slab and the three next ones"""
    corners = len(v0)
    y = v0[0::3, 1].astype(np.float64)
    slab = np.minimum(((y - y.min()) / max(y.max() - y.min(), 1e-9) * n_bones).astype(np.int64), n_bones - 1)
    slab = np.repeat(slab, 3)
    index = ((slab[:, None] + np.arange(4)[None, :]) % n_bones).astype(np.uint16)
    weight = np.zeros((corners, 4), dtype=f32)
    if kind == "rigid":
        weight[:, 0] = 1
    else:
        w = np.random.default_rng(seed).uniform(0.1, 1.0, (corners, 4))
        weight[:] = w / w.sum(axis=1)[:, None]
    return index, weight


def _rounds(arms, rounds, warm=2):
    names = list(arms)
    t = {k: [] for k in names}
    for k in range(rounds + warm):
        s = k % len(names)
        for arm in names[s:] + names[:s]:
            t0 = time.perf_counter()
            arms[arm]()
            if k >= warm:
                t[arm].append(1e3 * (time.perf_counter() - t0))
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)} for k, v in t.items()}


def measure(prt, name, rounds):
    import torch
    scene = _scene(prt, name)
    a = prt.scene_arrays(scene.desc)
    v0, n0 = a["vertices"].copy(), a["normals"].copy()
    T = int(scene.desc.triangle_count)
    out = {"triangles": T, "rounds": rounds, "skins": {}}
    for kind, n_bones in SKINS:
        r = prt.Renderer(scene.config(), device=0)
        r.upload_scene(scene)
        index, weight = influences(v0, kind, n_bones, 3)
        t0 = time.perf_counter()
        r.set_skin(v0, n0, index, weight, n_bones)
        set_ms = 1e3 * (time.perf_counter() - t0)
        M = bones(n_bones, 9)
        dM = torch.from_numpy(M).cuda()
        r.pose(M)
        pv, pn = r.read_posed()
        dv, dn = torch.from_numpy(pv).cuda(), torch.from_numpy(pn).cuda()
        torch.cuda.synchronize()
        bounds = r.read_bvh_bounds()
        r.update_vertices(dv, dn)
        same = bool(np.array_equal(bounds.view(np.uint32), r.read_bvh_bounds().view(np.uint32)))
        rec = {"set_skin_ms": round(set_ms, 2), "matrix_bytes": 48 * n_bones, "host_array_bytes": 96 * T, "device_bytes": 264 * T + 48 * n_bones,
               "same_bounds_as_update": same}
        rec["refit"] = _rounds({"pose_host_refit": lambda: r.pose(M), "pose_device_refit": lambda: r.pose(dM),
                                "update_device": lambda: r.update_vertices(dv, dn), "update_host": lambda: r.update_vertices(pv, pn)}, rounds)
        rec["rebuild"] = _rounds({"pose_host_rebuild": lambda: r.pose(M, rebuild=True), "pose_device_rebuild": lambda: r.pose(dM, rebuild=True),
                                  "rebuild_device": lambda: r.rebuild_bvh(dv, dn)}, max(rounds // 2, 3))
        m = rec["refit"]
        rec["pose_host_over_update_device"] = round(m["pose_host_refit"]["median_ms"] / m["update_device"]["median_ms"], 3)
        rec["pose_host_over_update_host"] = round(m["pose_host_refit"]["median_ms"] / m["update_host"]["median_ms"], 3)
        out["skins"]["%s_%d" % (kind, n_bones)] = rec
        r.close()
        print(json.dumps({name: {"%s_%d" % (kind, n_bones): rec}}), file=sys.stderr, flush=True)
    return out


def kernels_phase(prt, names):
    """the launches rocprofv3 times: KERNEL_CALLS poses per scene and skin, in the order of SKINS"""
    for name in names:
        scene = _scene(prt, name)
        a = prt.scene_arrays(scene.desc)
        v0, n0 = a["vertices"].copy(), a["normals"].copy()
        r = prt.Renderer(scene.config(), device=0)
        r.upload_scene(scene)
        for kind, n_bones in SKINS:
            index, weight = influences(v0, kind, n_bones, 3)
            r.set_skin(v0, n0, index, weight, n_bones)
            M = bones(n_bones, 9)
            for _ in range(KERNEL_CALLS):
                r.pose(M)
        r.close()


def kernel_times(prt, names, timeout):
    """per scene and skin: pose_kernel's duration (best and median of the calls after the first) and its streamed bytes per second"""
    rows = [r for r in kernel_rows(["--phase", "kernels", "--scenes", ",".join(names)], "pose", timeout) if "pose_kernel" in r[0]]
    assert len(rows) == KERNEL_CALLS * len(SKINS) * len(names), len(rows)
    out = {}
    for s, name in enumerate(names):
        T = int(_scene(prt, name).desc.triangle_count)
        out[name] = {}
        for k, (kind, n_bones) in enumerate(SKINS):
            first = (s * len(SKINS) + k) * KERNEL_CALLS
            us = [(e - b) / 1e3 for _, b, e in rows[first + 1:first + KERNEL_CALLS]]
            best = min(us)
            out[name]["%s_%d" % (kind, n_bones)] = {"pose_kernel_us_best": round(best, 2), "pose_kernel_us_median": round(float(np.median(us)), 2),
                                                    "streamed_bytes": 88 * 3 * T, "streamed_TB_per_s_best": round(88 * 3 * T / best / 1e6, 3),
                                                    "fraction_of_8_TB_per_s": round(88 * 3 * T / best / 1e6 / 8.0, 3)}
    out["note"] = "rocprofv3 --kernel-trace --stats, a run of its own; 88 streamed bytes per corner, the matrix table not counted"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_coat,cornell_dragon")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--phase", default="all", choices=["all", "rates", "kernels"])
    ap.add_argument("--rocprof-timeout", type=int, default=300)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
    names = a.scenes.split(",")
    if a.phase == "kernels":
        kernels_phase(prt, names)
        return
    doc = {"build_id": prt.build_id(), "scenes": {name: measure(prt, name, a.calls) for name in names}}
    if a.phase == "all":
        try:
            doc["kernel_time"] = kernel_times(prt, names, a.rocprof_timeout)
        except (subprocess.SubprocessError, AssertionError, KeyError, OSError) as e:
            doc["kernel_time"] = {"error": repr(e)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
