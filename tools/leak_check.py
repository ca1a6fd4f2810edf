#!/usr/bin/env python3
"""development helper: create / use / destroy many contexts; device memory must come back.

Every context renders; with --calls all (the default) it also goes through what allocates lazily and by lifetime: a vertex update and a
rebuild (host doors: the staging buffers, the refit tables, the spare tree set and the build's scratch), smoothing and motion on and off
(the topology, both snapshots), a primitive update, a host ray cast, a temporal denoise and a records denoise, and two more uploads of other
triangle counts (the primitives alone, then the mesh again) with a rebuild behind them, and a skin and a morph set with one pose of a morph
(host door: both sets' buffers and staging) before the skin is turned off, and the same set as planes (prt_set_morph_targets_layout: the
plane table in place of the per-corner one) with one morph before it is.  Prints the free-memory delta every 100 contexts and
one JSON line at the end.  A tool, not a test: free memory on a shared card is another tenant's business as much as ours.

    python tools/leak_check.py [--contexts 300] [--calls all|render]
"""
import argparse, importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
import torch
prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--contexts", type=int, default=300)
ap.add_argument("--calls", default="all", choices=["all", "render"])
args = ap.parse_args()
W, H = 160, 120
scene = prt.HostScene("cornell_coat.json"); cfg = scene.config(); seeds = prt.seed_pairs(64); cam = prt.default_camera(W, H)
a = prt.scene_arrays(scene.desc)
v0, n0 = a["vertices"].copy(), a["normals"].copy()
v1 = v0.copy(); v1[:, 1] += np.float32(0.01)
groups, n_groups = prt.weld_corners(v0)
n_meshes = int(scene.desc.object_count[7])
bare = prt.SceneDesc.from_buffer_copy(bytes(scene.desc))           # the primitives alone: another triangle count
bare.triangle_count, bare.bvh_node_count = 0, 0
rays = np.zeros((64, 8), dtype=np.float32); rays[:, 1] = 1.0; rays[:, 2] = 3.0; rays[:, 3] = 20.0; rays[:, 6] = -1.0
records = torch.zeros((H, W, 16), dtype=torch.float32, device="cuda")
bone_index = (np.arange(4 * len(v0)).reshape(-1, 4) % 4).astype(np.uint16)          # four bones, every corner under all of them
bone_weight = np.full((len(v0), 4), 0.25, dtype=np.float32)
matrices = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0.01, 0, 0, 1, 0], dtype=np.float32), (4, 1))
target = (np.arange(len(v0), dtype=np.uint32), v1 - v0, None)                       # one dense target
weights = np.array([0.5], dtype=np.float32)


def everything(r):
    r.update_vertices(v1, n0)
    r.set_motion(True)
    r.rebuild_bvh(v0, n0)
    r.set_smooth_normals(groups, n_groups, "area")
    r.update_vertices(v1, None)
    r.update_primitives(scene.desc.meshes, count=n_meshes)
    r.render_guides(1)
    r.denoise_temporal()
    r.export_denoise_inputs(records)
    r.denoise_records(records, W, H)
    r.denoise_records_temporal(records, W, H, cam)
    r.cast_rays(rays)
    r.set_smooth_normals(None)
    r.set_motion(False)
    r.upload_scene(bare)
    r.upload_scene(scene)
    r.rebuild_bvh(v1, None)
    r.set_skin(v0, n0, bone_index, bone_weight, 4)
    r.set_morph_targets(v0, n0, [target])
    r.pose_morphed(matrices, weights)
    r.set_skin(None)
    r.set_morph_targets(v0, n0, [target], layout="planes")
    r.morph(weights)
    r.set_morph_targets(None)


torch.cuda.synchronize()
free0 = torch.cuda.mem_get_info()[0]
delta = 0.0
for i in range(args.contexts):
    r = prt.Renderer(cfg, device=0); r.upload_scene(scene); r.set_camera(cam); r.resize(W, H)
    if i % 2: r.render_spp(2, seeds)
    else: r.render_frames(seeds[:32])
    if args.calls == "all": everything(r)
    r.read_framebuffer(); r.close()
    if i % 100 == 99 or i + 1 == args.contexts:
        delta = (free0 - torch.cuda.mem_get_info()[0]) / 1e6
        print(i + 1, "contexts, free delta MB", delta, flush=True)
print(json.dumps({"build_id": prt.build_id(), "contexts": args.contexts, "calls": args.calls, "free_delta_mb_after_last": delta}))
