#!/usr/bin/env python3
"""Temporal reprojection (prt_denoise_temporal) along a moving camera, against the spatial filter alone, on the MI355X.

For each scene: a yaw orbit of --frames frames (--yaw-step rad apart, the default camera's lens) at 1, 2 and 4 spp per frame, each frame
prt_reset + fresh paths + guides (K = 4) + prt_denoise_temporal (defaults): the loop of a moving camera.  Per setting: the per-frame wall time
(render + guides + temporal + filter, median over the frames after the first 4) and, at 4 cameras of the orbit, the RMSE against a 4096-spp
render of that camera next to the raw frame and to prt_denoise alone on the same frame.
Kernel time: tm_reproject_kernel and the rest of one call on cornell at the same size, from `rocprofv3 --kernel-trace --stats` in a run of its
own (this script with --phase kernels).  One JSON document on stdout (and into --out).

    python tools/temporal_rate.py [--width 1920 --height 1080] [--scenes cornell_diffuse,cornell_roughdiel] [--out profiles/r07_temporal.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _trace import kernel_rows      # noqa: E402

KERNEL_CALLS = 6


def _renderer(prt, variant, W, H):
    from conftest import VARIANTS, variant_config
    scene_json, phase, use_env = VARIANTS[variant]
    scene = prt.HostScene(scene_json)
    cfg = variant_config(scene, variant)
    cfg.phase_function = phase
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    if use_env:
        r.upload_envmap(prt.make_sky(64, 32))
    r.resize(W, H)
    return r, cfg


def _seeds(prt, cfg, spp, k):
    n = spp * max(cfg.max_bounces, 8) + 64
    return prt.seed_pairs(n, first_frame=1 + k * n)


def kernels_phase(prt, W, H, step):
    """the launches rocprofv3 times: KERNEL_CALLS frames of the orbit on cornell at 4 spp, each through prt_denoise_temporal"""
    r, cfg = _renderer(prt, "cornell_diffuse", W, H)
    for k in range(KERNEL_CALLS):
        r.set_camera(prt.orbit_camera(W, H, d_yaw=k * step))
        r.reset()
        r.render_spp(4, _seeds(prt, cfg, 4, k))
        r.render_guides(4)
        r.denoise_temporal()
    r.close()


def kernel_times(W, H, step, timeout):
    rows, stat_rows = kernel_rows(["--phase", "kernels", "--width", str(W), "--height", str(H), "--yaw-step", str(step)], "tm", timeout, with_stats=True)
    rows = [(name, e - b) for name, b, e in rows]
    stat_rows = [row for row in stat_rows if "tm_" in row.get("Name", "") or "dn_" in row.get("Name", "") or "guide_kernel" in row.get("Name", "")]
    call = [(name, ns) for name, ns in rows if "tm_" in name or "dn_" in name]
    per_call = 1 + 1 + 2 * 5 + 1                      # dn_var, tm_reproject, (gauss, atrous) x 5, tm_feedback
    assert len(call) == KERNEL_CALLS * per_call, len(call)
    calls = [call[c * per_call:(c + 1) * per_call] for c in range(KERNEL_CALLS)]
    totals = [sum(ns for _, ns in c) for c in calls]
    best = int(np.argmin(totals[1:])) + 1            # (call 0 has an empty history)
    one = calls[best]
    repro = [ns for c in calls[1:] for name, ns in c if "tm_reproject" in name]
    return {"temporal_call_ms": round(totals[best] / 1e6, 4),
            "parts_ms": {"dn_var": round(sum(ns for n, ns in one if "dn_var" in n) / 1e6, 4),
                         "tm_reproject": round(sum(ns for n, ns in one if "tm_reproject" in n) / 1e6, 4),
                         "tm_feedback": round(sum(ns for n, ns in one if "tm_feedback" in n) / 1e6, 4),
                         "gauss_total": round(sum(ns for n, ns in one if "gauss" in n) / 1e6, 4),
                         "atrous_total": round(sum(ns for n, ns in one if "atrous" in n) / 1e6, 4)},
            "tm_reproject_ms_min_median": [round(min(repro) / 1e6, 4), round(float(np.median(repro)) / 1e6, 4)],
            "rocprofv3_stats": stat_rows,
            "note": "kernel durations of one prt_denoise_temporal call with a history (best of %d), rocprofv3 --kernel-trace --stats"
                    % (KERNEL_CALLS - 1)}


def orbit(prt, a, variant, W, H):
    r, cfg = _renderer(prt, variant, W, H)
    F = a.frames
    sample = [F // 4 - 1, F // 2 - 1, 3 * F // 4 - 1, F - 1]
    cams = [prt.orbit_camera(W, H, d_yaw=k * a.yaw_step) for k in range(F)]
    refs = {}
    t0 = time.perf_counter()
    for k in sample:
        r.set_camera(cams[k])
        r.reset()
        r.render_spp(a.ref_spp, prt.seed_pairs(a.ref_spp * max(cfg.max_bounces, 8) + 64, first_frame=1000003))
        refs[k] = r.read_framebuffer()[..., :3].astype(np.float64)
    out = {"reference_s": round(time.perf_counter() - t0, 3), "sampled_frames": sample}

    # (a reference with non-finite pixels -- the rough dielectric has a few -- is compared on its finite ones; their count is reported)
    fin = {k: np.isfinite(v).all(-1) for k, v in refs.items()}
    out["reference_nonfinite_pixels"] = {str(k): int((~f).sum()) for k, f in fin.items()}

    def rmse(img, k):
        d = img[..., :3].astype(np.float64)[fin[k]] - refs[k][fin[k]]
        return float(np.sqrt(np.mean(d ** 2)))

    for spp in (1, 2, 4):
        r.reset_history()
        walls, rows = [], {}
        for k in range(F):
            r.synchronize()
            t = time.perf_counter()
            r.set_camera(cams[k])
            r.reset()
            r.render_spp(spp, _seeds(prt, cfg, spp, k))
            r.render_guides(4)
            img = r.denoise_temporal()
            r.synchronize()
            walls.append(time.perf_counter() - t)
            if k in refs:
                raw = r.read_framebuffer()
                rows[str(k)] = {"raw": rmse(raw, k), "spatial": rmse(r.denoise(), k), "temporal": rmse(img, k),
                                "nonfinite_raw_temporal": [int((~np.isfinite(raw[..., :3]).all(-1)).sum()), int((~np.isfinite(img[..., :3]).all(-1)).sum())]}
        last = rows[str(F - 1)]
        out["spp%d" % spp] = {"frame_wall_ms_median": round(1e3 * float(np.median(walls[4:])), 3), "rmse": rows,
                              "temporal_over_spatial_last": round(last["temporal"] / last["spatial"], 3),
                              "temporal_over_spatial_mean": round(float(np.mean([v["temporal"] / v["spatial"] for v in rows.values()])), 3)}
        print(json.dumps({variant: {"spp%d" % spp: out["spp%d" % spp]}}), file=sys.stderr, flush=True)
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scenes", default="cornell_diffuse,cornell_roughdiel")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--yaw-step", type=float, default=0.01)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--phase", default="all", choices=["all", "quality", "kernels"])
    ap.add_argument("--rocprof-timeout", type=int, default=600)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
    W, H = a.width, a.height
    if a.phase == "kernels":
        kernels_phase(prt, W, H, a.yaw_step)
        return
    doc = {"width": W, "height": H, "frames": a.frames, "yaw_step_rad": a.yaw_step, "ref_spp": a.ref_spp, "guide_spp": 4,
           "build_id": prt.build_id(), "filter": dict(prt.DENOISE_DEFAULTS), "temporal": dict(prt.TEMPORAL_DEFAULTS)}
    doc["orbit"] = {v: orbit(prt, a, v, W, H) for v in a.scenes.split(",")}
    if a.phase == "all":
        try:
            doc["kernel_time"] = kernel_times(W, H, a.yaw_step, a.rocprof_timeout)
        except (subprocess.SubprocessError, AssertionError, KeyError, OSError) as e:
            doc["kernel_time"] = {"error": repr(e)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
