#!/usr/bin/env python3
"""prt_update_primitives (spheres, quads and SDF primitives moved in place) against what the same change cost before it existed, on the MI355X.

Per scene (cornell_coat and the 871 k-triangle stand-in of BASELINE config 5): the light sphere is moved a little, and timed, wall clock, each
call complete on return, the two doors alternated call by call and the upload in a phase of its own behind them, medians over --calls rounds:
  update_device      prt_update_primitives_device from a device buffer of records
  update_host        prt_update_primitives from host records (PCIe included)
  upload_scene       the parent's only way to move a primitive: prt_upload_scene of the moved scene
and, with prt_set_motion on, prt_render_guides (4 samples) at 1920x1080 after a vertex update alone (the triangle-only motion instance),
after a primitive update alone and after both (the primitive-motion instances, without and with the triangle term).
These are measurements to write down: there is no pass mark.  One JSON document on stdout (and into --out).

    python tools/update_primitives_rate.py [--scenes cornell_coat,cornell_dragon] [--out profiles/r19_update_primitives.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MESH_BYTES = 256
POS_OFFSET = 64             # prt_mesh::pos (include/prt_types.h)


def _scene(prt, name):
    if "dragon" in name:
        prt.ensure_dragon_standin()
    return prt.HostScene(name + ".json")


def _records(desc):
    n = int(desc.object_count[7])
    return np.frombuffer((C.c_uint8 * (MESH_BYTES * n)).from_address(desc.meshes), dtype=np.uint8).copy().reshape(n, MESH_BYTES)


def _moved(rec, k):
    """mesh 0 (the light sphere of the cornell scenes) pushed along x by a few millimetres, alternating"""
    out = rec.copy()
    pos = out[0, POS_OFFSET:POS_OFFSET + 12].view(np.float32)
    pos[0] += np.float32(0.002 * (1 + k % 2))
    return out


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def _stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}


def measure(prt, name, rounds, width=1920, height=1080):
    import torch
    scene = _scene(prt, name)
    cfg = scene.config()
    rec = _records(scene.desc)
    poses = [_moved(rec, k) for k in range(2)]
    dev = [torch.from_numpy(p).cuda() for p in poses]
    descs = []
    for p in poses:
        d = prt.SceneDesc.from_buffer_copy(bytes(scene.desc))
        d.meshes = p.ctypes.data
        descs.append(d)
    torch.cuda.synchronize()
    upd, up = prt.Renderer(cfg, device=0), prt.Renderer(cfg, device=0)
    for r in (upd, up):
        r.upload_scene(scene)
    t = {"update_device": [], "update_host": [], "upload_scene": []}
    arms = {"update_device": lambda k: upd.update_primitives(dev[k % 2]), "update_host": lambda k: upd.update_primitives(poses[k % 2])}
    names = list(arms)
    for k in range(rounds + 2):
        for arm in names[k % 2:] + names[:k % 2]:                          # (the two doors alternate, the order swaps)
            ms = _timed(lambda: arms[arm](k))
            if k >= 2:                                                     # (two warm-up rounds: allocations, first launches)
                t[arm].append(ms)
    # the upload in a phase of its own: it frees and allocates every buffer of a scene, and what the runtime defers of that lands on the next
    # call of the process, whichever context makes it (taken in turn with the doors, a 0.06 ms update read 20 ms after an 871 k-triangle upload)
    for k in range(max(rounds // 2, 3) + 1):
        ms = _timed(lambda: (up.upload_scene(descs[k % 2]), up.synchronize()))
        if k >= 1:
            t["upload_scene"].append(ms)
    for r in (upd, up):
        r.close()
    out = {"triangles": int(scene.desc.triangle_count), "primitives": int(scene.desc.object_count[7]), "rounds": rounds,
           "record_bytes": MESH_BYTES * int(scene.desc.object_count[7])}
    for arm, v in t.items():
        out[arm] = _stats(v)
    out["upload_scene_over_update_device_median"] = round(out["upload_scene"]["median_ms"] / out["update_device"]["median_ms"], 1)
    out["upload_scene_over_update_host_median"] = round(out["upload_scene"]["median_ms"] / out["update_host"]["median_ms"], 1)

    # the guide render: which instance runs is decided by the snapshots pending
    a = prt.scene_arrays(scene.desc)
    v0, n0 = a["vertices"].copy(), a["normals"].copy()
    dv = []
    for k in range(2):
        v = v0.copy()
        v[:, 0] += np.float32(0.001 * (1 + k))
        dv.append(torch.from_numpy(v).cuda())
    dn = torch.from_numpy(n0).cuda()
    torch.cuda.synchronize()
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    r.set_camera(prt.default_camera(width, height))
    r.resize(width, height)
    r.set_motion(True)
    g = {"none_pending": [], "triangles_only": [], "primitives_only": [], "both": []}
    tri = int(scene.desc.triangle_count) > 0
    n_v = n_p = 0                                                          # (every update changes the pose: the poses alternate per call)
    for k in range(rounds + 2):
        for arm in g:
            if arm in ("triangles_only", "both") and tri:
                n_v += 1
                r.update_vertices(dv[n_v % 2], dn)
            if arm in ("primitives_only", "both"):
                n_p += 1
                r.update_primitives(dev[n_p % 2])
            ms = _timed(lambda: r.render_guides(4))
            if k >= 2:
                g[arm].append(ms)
    moving = float((np.abs(r.read_motion()[..., :3]).max(-1) > 0).mean())
    r.close()
    out["render_guides"] = {"frame": [width, height], "samples": 4, "pixels_with_motion_after_both": round(moving, 4)}
    for arm, v in g.items():
        out["render_guides"][arm] = _stats(v)
    out["render_guides"]["primitives_only_minus_triangles_only_median_ms"] = round(
        out["render_guides"]["primitives_only"]["median_ms"] - out["render_guides"]["triangles_only"]["median_ms"], 4)
    out["render_guides"]["both_minus_triangles_only_median_ms"] = round(
        out["render_guides"]["both"]["median_ms"] - out["render_guides"]["triangles_only"]["median_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell_coat,cornell_dragon")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
    doc = {"build_id": prt.build_id(), "scenes": {}}
    for name in a.scenes.split(","):
        doc["scenes"][name] = measure(prt, name, a.calls)
        print(json.dumps({name: doc["scenes"][name]}), file=sys.stderr, flush=True)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
