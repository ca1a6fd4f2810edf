#!/usr/bin/env python3
"""prt_morph / prt_pose_morphed (the mesh morphed on the device from target weights) against the parent's routes to the same scene, on the
MI355X.

Per scene (the teapot of cornell_coat and the 871 k-triangle stand-in of cornell_dragon) and per target set (1, 8 and 64 targets, each over
a random 5 % and over 100 % of the corners, all weights active), wall clock per call, each call complete on return, the arms of one group
alternated call by call with a rotating order, medians over --calls rounds:
  morph_host / morph_device                  prt_morph (n_targets x 4 bytes from host memory) / prt_morph_device, PRT_POSE_REFIT
  update_device / update_host                the parent's routes: prt_update_vertices_device from device buffers holding prt_read_morphed's
                                             arrays / prt_update_vertices from host arrays (PCIe included)
  pose / pose_morphed_zero / pose_morphed    prt_pose on a skin of 16 bones with four influences per corner whose rest pose is the base, and
                                             prt_pose_morphed on the same skin with all weights zero (the price of the table) and active
Kernel time: morph_kernel's and pose_morphed_kernel's durations from `rocprofv3 --kernel-trace --stats` in a run of its own (this script
with --phase kernels), and their streamed bytes per second (per corner 16 + 16 + 8 in and 32 out, 32 per entry; the fused kernel 24 more per
corner for its indices and weights; the weight and matrix tables are not counted).  One JSON document on stdout (and into --out).  There is
no pass mark.

--layout both: the two table layouts of prt_set_morph_targets_layout against each other instead, per scene and set on two contexts of one
process that hold the same set, PRT_MORPH_LAYOUT_CORNERS (the parent's kernel) and PRT_MORPH_LAYOUT_PLANES:
  corners / planes                           prt_morph_device, PRT_POSE_REFIT, the two arms alternated call by call; medians with the
                                             interquartile range; set time, prt_get_morph_report (table_bytes, fill) and device bytes of both
  active targets                             the last dense set of --sets with k = 0, 1, 8, ... of its weights non-zero (--active), both arms,
                                             and a plane set of one target without entries: a morph that reads no plane
Kernel time: the four kernels' durations in a profiler run of their own with the same alternation, medians with the interquartile range,
and the bytes each streams per second: per corner 64 (16 + 16 in, 32 out) and the table -- CORNERS 8 per corner of offsets and 32 per
entry, PLANES 4 per block and, per plane of an active target, 16 + 1536 (the head and six rows; 16 for a plane that is skipped).
dense_condition: the plane kernel's median below the per-corner kernel's by more than the two interquartile ranges together.

    python tools/morph_rate.py [--scenes cornell_coat,cornell_dragon] [--out profiles/r23_morph.json]
    python tools/morph_rate.py --layout both --scenes cornell_dragon --out profiles/r28_morph_planes.json
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
from pose_rate import _rounds, _scene, bones, influences      # noqa: E402

KERNEL_CALLS = 5
SETS = [(1, 0.05), (8, 0.05), (64, 0.05), (1, 1.0), (8, 1.0), (64, 1.0)]
N_BONES = 16
f32 = np.float32


def target_set(corners, n_targets, fraction, seed):
    """n_targets targets over `fraction` of the corners each (a random subset per target; the dense targets share one pair of delta arrays),
    and weights that are all active"""
    rng = np.random.default_rng(seed)
    k = corners if fraction >= 1.0 else max(1, int(round(fraction * corners)))
    dp = np.zeros((k, 4), dtype=f32)
    dn = np.zeros((k, 4), dtype=f32)
    dp[:, :3], dn[:, :3] = rng.uniform(-0.01, 0.01, (k, 3)), rng.uniform(-0.1, 0.1, (k, 3))
    everything = np.arange(corners, dtype=np.uint32)
    targets = []
    for _ in range(n_targets):
        corner = everything if k == corners else np.sort(rng.choice(corners, size=k, replace=False)).astype(np.uint32)
        targets.append((corner, dp, dn))
    return targets, np.full(n_targets, 0.5 / n_targets, dtype=f32), k * n_targets


def _name(n_targets, fraction):
    return "%d_targets_%d_percent" % (n_targets, int(round(100 * fraction)))


def measure(prt, name, rounds, sets):
    import torch
    scene = _scene(prt, name)
    a = prt.scene_arrays(scene.desc)
    v0, n0 = a["vertices"].copy(), a["normals"].copy()
    T = int(scene.desc.triangle_count)
    out = {"triangles": T, "rounds": rounds, "sets": {}}
    index, weight = influences(v0, "four", N_BONES, 3)
    M = bones(N_BONES, 9)
    for n_targets, fraction in sets:
        r = prt.Renderer(scene.config(), device=0)
        r.upload_scene(scene)
        targets, w, entries = target_set(3 * T, n_targets, fraction, 5)
        t0 = time.perf_counter()
        r.set_morph_targets(v0, n0, targets)
        set_ms = 1e3 * (time.perf_counter() - t0)
        dw = torch.from_numpy(w).cuda()
        r.morph(w)
        pv, pn = r.read_morphed()
        dv, dn = torch.from_numpy(pv).cuda(), torch.from_numpy(pn).cuda()
        torch.cuda.synchronize()
        bounds = r.read_bvh_bounds()
        r.update_vertices(dv, dn)
        same = bool(np.array_equal(bounds.view(np.uint32), r.read_bvh_bounds().view(np.uint32)))
        rec = {"set_morph_targets_ms": round(set_ms, 2), "entries": entries, "weight_bytes": 4 * n_targets, "host_array_bytes": 96 * T,
               "device_bytes": (192 + 12) * T + 32 * entries + 4 * n_targets, "same_bounds_as_update": same}
        rec["morph"] = _rounds({"morph_host": lambda: r.morph(w), "morph_device": lambda: r.morph(dw),
                                "update_device": lambda: r.update_vertices(dv, dn), "update_host": lambda: r.update_vertices(pv, pn)}, rounds)
        r.set_skin(v0, n0, index, weight, N_BONES)
        zero = np.zeros_like(w)
        rec["fused"] = _rounds({"pose": lambda: r.pose(M), "pose_morphed_zero": lambda: r.pose_morphed(M, zero),
                                "pose_morphed": lambda: r.pose_morphed(M, w)}, rounds)
        m, f = rec["morph"], rec["fused"]
        rec["morph_host_over_update_device"] = round(m["morph_host"]["median_ms"] / m["update_device"]["median_ms"], 3)
        rec["morph_host_over_update_host"] = round(m["morph_host"]["median_ms"] / m["update_host"]["median_ms"], 3)
        rec["pose_morphed_zero_over_pose"] = round(f["pose_morphed_zero"]["median_ms"] / f["pose"]["median_ms"], 3)
        rec["pose_morphed_over_pose"] = round(f["pose_morphed"]["median_ms"] / f["pose"]["median_ms"], 3)
        out["sets"][_name(n_targets, fraction)] = rec
        r.close()
        print(json.dumps({name: {_name(n_targets, fraction): rec}}), file=sys.stderr, flush=True)
    return out


def kernels_phase(prt, names, sets):
    """the launches rocprofv3 times: KERNEL_CALLS morphs, then KERNEL_CALLS fused poses, per scene and set, in the order of `sets`"""
    for name in names:
        scene = _scene(prt, name)
        a = prt.scene_arrays(scene.desc)
        v0, n0 = a["vertices"].copy(), a["normals"].copy()
        T = int(scene.desc.triangle_count)
        r = prt.Renderer(scene.config(), device=0)
        r.upload_scene(scene)
        index, weight = influences(v0, "four", N_BONES, 3)
        r.set_skin(v0, n0, index, weight, N_BONES)
        M = bones(N_BONES, 9)
        for n_targets, fraction in sets:
            targets, w, _ = target_set(3 * T, n_targets, fraction, 5)
            r.set_morph_targets(v0, n0, targets)
            for _ in range(KERNEL_CALLS):
                r.morph(w)
            for _ in range(KERNEL_CALLS):
                r.pose_morphed(M, w)
        r.close()


def kernel_times(prt, names, sets, timeout):
    """per scene and set: the two kernels' durations (best and median of the calls after the first) and their streamed bytes per second"""
    spec = ",".join("%d:%g" % s for s in sets)
    rows = kernel_rows(["--phase", "kernels", "--scenes", ",".join(names), "--sets", spec], "morph", timeout)
    out = {}
    for kernel, per_corner in (("morph_kernel", 72), ("pose_morphed_kernel", 96)):
        mine = [r for r in rows if kernel in r[0] and (kernel != "morph_kernel" or "pose_morphed" not in r[0])]
        assert len(mine) == KERNEL_CALLS * len(sets) * len(names), (kernel, len(mine))
        for s, name in enumerate(names):
            T = int(_scene(prt, name).desc.triangle_count)
            for k, (n_targets, fraction) in enumerate(sets):
                entries = n_targets * (3 * T if fraction >= 1.0 else max(1, int(round(fraction * 3 * T))))
                first = (s * len(sets) + k) * KERNEL_CALLS
                us = [(e - b) / 1e3 for _, b, e in mine[first + 1:first + KERNEL_CALLS]]
                best, streamed = min(us), per_corner * 3 * T + 32 * entries
                out.setdefault(name, {}).setdefault(_name(n_targets, fraction), {})[kernel] = {
                    "us_best": round(best, 2), "us_median": round(float(np.median(us)), 2), "streamed_bytes": streamed,
                    "streamed_TB_per_s_best": round(streamed / best / 1e6, 3)}
    out["note"] = "rocprofv3 --kernel-trace --stats, a run of its own; per corner 72 (fused: 96) streamed bytes and 32 per entry, the weight and matrix tables not counted"
    return out


# ---- --layout both: PRT_MORPH_LAYOUT_CORNERS against PRT_MORPH_LAYOUT_PLANES ----------------------------------------------------------------

LAYOUTS = ("corners", "planes")
KERNEL_OF = {"corners": ("morph_kernel", "pose_morphed_kernel"), "planes": ("morph_planes_kernel", "pose_morphed_planes_kernel")}


def _spread(values):
    q1, med, q3 = np.percentile(np.asarray(values, dtype=np.float64), [25, 50, 75])
    return {"median": round(float(med), 4), "iqr": round(float(q3 - q1), 4), "min": round(float(min(values)), 4), "n": len(values)}


def _alternated(arms, rounds, warm=2):
    """pose_rate._rounds with the spread: wall clock in ms per arm, the arms alternated call by call with a rotating order"""
    names = list(arms)
    t = {k: [] for k in names}
    for k in range(rounds + warm):
        s = k % len(names)
        for arm in names[s:] + names[:s]:
            t0 = time.perf_counter()
            arms[arm]()
            if k >= warm:
                t[arm].append(1e3 * (time.perf_counter() - t0))
    return {k: _spread(v) for k, v in t.items()}


def active_weights(n_targets, k):
    """k of the n_targets weights non-zero, spread over the set"""
    w = np.zeros(n_targets, dtype=f32)
    if k:
        w[np.linspace(0, n_targets - 1, k).round().astype(np.int64)] = 0.5 / k
    return w


def _pair(prt, scene, v0, n0, targets):
    """two contexts over the scene that hold the same set, one per layout: ({layout: Renderer}, {layout: set time in ms})"""
    pair, set_ms = {}, {}
    for layout in LAYOUTS:
        r = prt.Renderer(scene.config(), device=0)
        r.upload_scene(scene)
        t0 = time.perf_counter()
        r.set_morph_targets(v0, n0, targets, layout=layout)
        set_ms[layout] = round(1e3 * (time.perf_counter() - t0), 2)
        pair[layout] = r
    return pair, set_ms


def _active_set(sets, active):
    """the set the active-targets arm runs over: the last dense one, and the k that fit it"""
    dense = [s for s in sets if s[1] >= 1.0]
    if not dense or not active:
        return None, []
    return dense[-1], [k for k in active if k <= dense[-1][0]]


def _empty_target():
    return [(np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=f32), None)]


def measure_layouts(prt, name, rounds, sets, active):
    import torch
    scene = _scene(prt, name)
    a = prt.scene_arrays(scene.desc)
    v0, n0 = a["vertices"].copy(), a["normals"].copy()
    T = int(scene.desc.triangle_count)
    out = {"triangles": T, "rounds": rounds, "sets": {}}
    act_set, ks = _active_set(sets, active)
    for n_targets, fraction in sets:
        targets, w, entries = target_set(3 * T, n_targets, fraction, 5)
        pair, set_ms = _pair(prt, scene, v0, n0, targets)
        dw = torch.from_numpy(w).cuda()
        rec = {"entries": entries, "set_morph_targets_ms": set_ms, "report": {}, "device_bytes": {}}
        morphed = {}
        for layout, r in pair.items():
            rep = r.morph_report()
            rec["report"][layout] = rep
            rec["device_bytes"][layout] = 192 * T + rep["table_bytes"] + 4 * n_targets
            r.morph(dw)
            morphed[layout] = r.read_morphed()
        rec["same_bytes"] = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(morphed["corners"], morphed["planes"]))
        del morphed
        rec["morph_device_ms"] = _alternated({layout: (lambda r=r: r.morph(dw)) for layout, r in pair.items()}, rounds)
        if (n_targets, fraction) == act_set:
            rec["active"] = {}
            for k in ks:
                dk = torch.from_numpy(active_weights(n_targets, k)).cuda()
                rec["active"]["k_%d" % k] = _alternated({layout: (lambda r=r: r.morph(dk)) for layout, r in pair.items()}, rounds)
            r = pair["planes"]
            r.set_morph_targets(v0, n0, _empty_target(), layout="planes")
            d1 = torch.zeros(4, dtype=torch.float32, device="cuda")
            rec["active"]["one_empty_target"] = _alternated({"planes": lambda: r.morph(d1)}, rounds)
        for r in pair.values():
            r.close()
        out["sets"][_name(n_targets, fraction)] = rec
        print(json.dumps({name: {_name(n_targets, fraction): rec}}), file=sys.stderr, flush=True)
    return out


def layout_kernels_phase(prt, names, sets, active, rounds):
    """the launches rocprofv3 times, per scene and set: `rounds` morphs alternated between the layouts, `rounds` fused poses likewise, and for
    the active-targets set `rounds` alternated morphs per k and `rounds` morphs over the plane set of one empty target"""
    import torch
    act_set, ks = _active_set(sets, active)
    for name in names:
        scene = _scene(prt, name)
        a = prt.scene_arrays(scene.desc)
        v0, n0 = a["vertices"].copy(), a["normals"].copy()
        T = int(scene.desc.triangle_count)
        index, weight = influences(v0, "four", N_BONES, 3)
        M = torch.from_numpy(bones(N_BONES, 9)).cuda()
        for n_targets, fraction in sets:
            targets, w, _ = target_set(3 * T, n_targets, fraction, 5)
            pair, _ = _pair(prt, scene, v0, n0, targets)
            dw = torch.from_numpy(w).cuda()
            for r in pair.values():
                r.set_skin(v0, n0, index, weight, N_BONES)
            for _ in range(rounds):
                for r in pair.values():
                    r.morph(dw)
            for _ in range(rounds):
                for r in pair.values():
                    r.pose_morphed(M, dw)
            if (n_targets, fraction) == act_set:
                for k in ks:
                    dk = torch.from_numpy(active_weights(n_targets, k)).cuda()
                    for _ in range(rounds):
                        for r in pair.values():
                            r.morph(dk)
                r = pair["planes"]
                r.set_morph_targets(v0, n0, _empty_target(), layout="planes")
                d1 = torch.zeros(4, dtype=torch.float32, device="cuda")
                for _ in range(rounds):
                    r.morph(d1)
            for r in pair.values():
                r.close()


def layout_kernel_times(prt, names, sets, active, rounds, timeout, doc):
    """per scene and set: the four kernels' durations (median, interquartile range and best of the calls after the first) and their streamed
    bytes per second; the active-targets curves; the dense condition"""
    spec = ",".join("%d:%g" % s for s in sets)
    rows = kernel_rows(["--phase", "kernels", "--layout", "both", "--scenes", ",".join(names), "--sets", spec, "--calls", str(rounds),
                        "--active", ",".join(str(k) for k in active)], "morph_planes", timeout)
    act_set, ks = _active_set(sets, active)
    mine = {kernel: [(e - b) / 1e3 for n, b, e in rows if kernel + "(" in n or n.endswith(kernel) or ("prt::" + kernel) in n or ("3prt%d%s" % (len(kernel), kernel)) in n]
            for layout in LAYOUTS for kernel in KERNEL_OF[layout]}
    at = {kernel: 0 for kernel in mine}

    def take(kernel, streamed):
        us = mine[kernel][at[kernel] + 1:at[kernel] + rounds]                             # (the first call of a run is left out)
        assert len(us) == rounds - 1, (kernel, at[kernel], len(mine[kernel]))
        at[kernel] += rounds
        rec = _spread(us)
        rec = {"us_median": rec["median"], "us_iqr": rec["iqr"], "us_best": rec["min"], "streamed_bytes": int(streamed)}
        rec["streamed_TB_per_s_median"] = round(streamed / rec["us_median"] / 1e6, 3) if rec["us_median"] else None
        return rec
    out = {}
    for name in names:
        T = doc["scenes"][name]["triangles"]
        for n_targets, fraction in sets:
            key = _name(n_targets, fraction)
            rep = doc["scenes"][name]["sets"][key]["report"]
            entries, planes = rep["planes"]["entries"], rep["planes"]["planes"]
            streamed = {"corners": (64 + 8) * 3 * T + 32 * entries, "planes": 64 * 3 * T + 4 * ((3 * T + 63) // 64 + 1) + (16 + 1536) * planes}
            rec = {}
            for fused in (0, 1):
                for layout in LAYOUTS:
                    rec[KERNEL_OF[layout][fused]] = take(KERNEL_OF[layout][fused], streamed[layout] + 24 * 3 * T * fused)
            c, p = rec["morph_kernel"], rec["morph_planes_kernel"]
            rec["planes_over_corners"] = round(p["us_median"] / c["us_median"], 4)
            if fraction >= 1.0 and n_targets > 1:
                rec["dense_condition"] = {"holds": bool(c["us_median"] - p["us_median"] > c["us_iqr"] + p["us_iqr"]),
                                          "corners_minus_planes_us": round(c["us_median"] - p["us_median"], 3),
                                          "combined_iqr_us": round(c["us_iqr"] + p["us_iqr"], 3)}
            if (n_targets, fraction) == act_set:
                rec["active"] = {}
                per_target = planes // n_targets
                for k in ks:
                    sk = 64 * 3 * T + 4 * ((3 * T + 63) // 64 + 1) + 16 * planes + 1536 * per_target * k
                    rec["active"]["k_%d" % k] = {"morph_kernel": take("morph_kernel", streamed["corners"]), "morph_planes_kernel": take("morph_planes_kernel", sk)}
                rec["active"]["one_empty_target"] = {"morph_planes_kernel": take("morph_planes_kernel", 64 * 3 * T + 4 * ((3 * T + 63) // 64 + 1))}
            out.setdefault(name, {})[key] = rec
    out["note"] = ("rocprofv3 --kernel-trace --stats, a run of its own, the layouts alternated call by call; streamed bytes: 64 per corner and the "
                   "table (CORNERS: 8 per corner and 32 per entry; PLANES: 4 per block, 16 per plane and 1536 per plane of an active target), "
                   "the fused kernels 24 more per corner; the weight and matrix tables not counted")
    return out


def main_layouts(prt, a, names, sets):
    active = [int(k) for k in a.active.split(",") if k != ""]
    if a.phase == "kernels":
        layout_kernels_phase(prt, names, sets, active, a.calls)
        return
    doc = {"build_id": prt.build_id(), "layout": "both", "scenes": {name: measure_layouts(prt, name, a.calls, sets, active) for name in names}}
    if a.phase == "all":
        try:
            doc["kernel_time"] = layout_kernel_times(prt, names, sets, active, a.calls, a.rocprof_timeout, doc)
        except (subprocess.SubprocessError, AssertionError, KeyError, OSError) as e:
            doc["kernel_time"] = {"error": repr(e)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", default="corners", choices=["corners", "both"], help="both: the two table layouts against each other")
    ap.add_argument("--active", default="0,1,8,64", help="--layout both: the numbers of non-zero weights of the active-targets arm")
    ap.add_argument("--scenes", default="cornell_coat,cornell_dragon")
    ap.add_argument("--sets", default=",".join("%d:%g" % s for s in SETS), help="n_targets:fraction, ...")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--phase", default="all", choices=["all", "rates", "kernels"])
    ap.add_argument("--rocprof-timeout", type=int, default=300)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
    names = a.scenes.split(",")
    sets = [(int(s.split(":")[0]), float(s.split(":")[1])) for s in a.sets.split(",")]
    if a.layout == "both":
        main_layouts(prt, a, names, sets)
        return
    if a.phase == "kernels":
        kernels_phase(prt, names, sets)
        return
    doc = {"build_id": prt.build_id(), "scenes": {name: measure(prt, name, a.calls, sets) for name in names}}
    if a.phase == "all":
        try:
            doc["kernel_time"] = kernel_times(prt, names, sets, a.rocprof_timeout)
        except (subprocess.SubprocessError, AssertionError, KeyError, OSError) as e:
            doc["kernel_time"] = {"error": repr(e)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
