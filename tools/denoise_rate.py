#!/usr/bin/env python3
"""The denoiser (prt_render_guides + prt_denoise) against fixed samples per pixel, on the MI355X.

Quality: for each scene a reference render (4096 spp with other seeds), fixed 1024 spp as the yardstick, and 4 / 16 / 64 / 256 spp rendered
adaptively with min_spp = max_spp = N, rel_err = 0 (the "N spp" picture plus its stats plane), each raw and denoised with both variance
sources.  Per row: wall time (render, + guides at K = 4 and the filter for the denoised rows) and RMSE against the reference.
Kernel time: the guide kernel at K = 1 / 4 / 16 and the filter at 5 passes, at the same size on cornell (BASELINE config 2) and through the
871 k-triangle tree (config 5's scene), from `rocprofv3 --kernel-trace --stats` in a run of its own (this script with --phase kernels).
One JSON document on stdout (and into --out).

    python tools/denoise_rate.py [--width 1920 --height 1080] [--scenes cornell_diffuse,cornell_roughdiel] [--out profiles/r06_denoise.json]
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

GUIDE_K = (1, 4, 16)
REPS = 3
KERNEL_SCENES = ("cornell_diffuse.json", "cornell_dragon.json")


def _renderer(prt, scene_json, W, H, variant=None):
    from conftest import VARIANTS, variant_camera, variant_config
    if variant:
        scene_json, phase, use_env = VARIANTS[variant]
    else:
        phase, use_env = 0, False
    if "dragon" in scene_json:
        prt.ensure_dragon_standin()
    scene = prt.HostScene(scene_json)
    cfg = variant_config(scene, variant) if variant else scene.config()
    cfg.phase_function = phase
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    if use_env:
        r.upload_envmap(prt.make_sky(64, 32))
    r.set_camera(variant_camera(prt, variant, W, H) if variant else prt.default_camera(W, H))
    r.resize(W, H)
    return r


def kernels_phase(prt, W, H):
    """the launches rocprofv3 times, in a fixed order: per scene, REPS x guides at each K, then REPS x the filter (stats)"""
    for scene_json in KERNEL_SCENES:
        r = _renderer(prt, scene_json, W, H)
        r.reset()
        r.render_adaptive(prt.seed_pairs(4 * 64 + 64), 4, 4, 0.0)
        for k in GUIDE_K:
            for _ in range(REPS):
                r.render_guides(k)
        for _ in range(REPS):
            r.denoise(var_source="stats")
        r.close()


def kernel_times(W, H, timeout):
    rows, stat_rows = kernel_rows(["--phase", "kernels", "--width", str(W), "--height", str(H)], "dn", timeout, with_stats=True)
    rows = [(name, e - b) for name, b, e in rows]
    stat_rows = [row for row in stat_rows if "guide_kernel" in row.get("Name", "") or "dn_" in row.get("Name", "")]
    guides = [ns for name, ns in rows if "guide_kernel" in name]
    filt = [(name, ns) for name, ns in rows if "dn_" in name]
    per_scene = REPS * len(GUIDE_K)
    per_denoise = 1 + 2 * 5
    assert len(guides) == per_scene * len(KERNEL_SCENES) and len(filt) == REPS * per_denoise * len(KERNEL_SCENES), (len(guides), len(filt))
    out = {}
    for si, scene_json in enumerate(KERNEL_SCENES):
        g = guides[si * per_scene:(si + 1) * per_scene]
        f = filt[si * REPS * per_denoise:(si + 1) * REPS * per_denoise]
        res = {"guides_ms": {"K%d" % k: round(min(g[j * REPS:(j + 1) * REPS]) / 1e6, 4) for j, k in enumerate(GUIDE_K)}}
        calls = [sum(ns for _, ns in f[c * per_denoise:(c + 1) * per_denoise]) for c in range(REPS)]
        best = int(np.argmin(calls))
        one = f[best * per_denoise:(best + 1) * per_denoise]
        res["filter_5_passes_ms"] = round(calls[best] / 1e6, 4)
        res["filter_parts_ms"] = {"var": round(one[0][1] / 1e6, 4),
                                  "gauss_total": round(sum(ns for name, ns in one if "gauss" in name) / 1e6, 4),
                                  "atrous_per_pass": [round(ns / 1e6, 4) for name, ns in one if "atrous" in name]}
        out[scene_json.replace(".json", "")] = res
    out["rocprofv3_stats"] = stat_rows
    out["note"] = ("sum of the kernel durations of one call (best of %d), from rocprofv3 --kernel-trace --stats; guides: one launch per call. "
                   "The scene is rendered at 4 spp first so that the filter has a picture and a stats plane" % REPS)
    return out


def quality(prt, a, W, H):
    doc = {}
    for variant in a.scenes.split(","):
        r = _renderer(prt, None, W, H, variant=variant)

        def timed(fn, reset=True):
            if reset:
                r.reset()
            r.synchronize()
            t0 = time.perf_counter()
            res = fn()
            r.synchronize()
            return time.perf_counter() - t0, res

        ref_seeds = prt.seed_pairs(a.ref_spp * 16 + 64, first_frame=1000003)
        t_ref, _ = timed(lambda: r.render_spp(a.ref_spp, ref_seeds))
        ref = r.read_framebuffer()[..., :3].astype(np.float64)

        def rmse(img):
            return float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - ref) ** 2)))

        seeds = prt.seed_pairs(1024 * 16 + 64)
        t_fix, _ = timed(lambda: r.render_spp(1024, seeds))
        out = {"reference_s": round(t_ref, 3), "fixed_1024": {"wall_s": round(t_fix, 4), "rmse": rmse(r.read_framebuffer())}}
        t_guides, _ = timed(lambda: r.render_guides(4), reset=False)
        out["guides_k4_wall_s"] = round(t_guides, 4)
        rows = {}
        for spp in [int(x) for x in a.spp.split(",")]:
            t, _ = timed(lambda: r.render_adaptive(seeds, spp, spp, 0.0))
            row = {"render_wall_s": round(t, 4), "raw_rmse": rmse(r.read_framebuffer())}
            for source in ("stats", "spatial"):
                td, img = timed(lambda: r.denoise(var_source=source), reset=False)
                row["denoised_%s" % source] = {"filter_wall_s": round(td, 4), "wall_s": round(t + t_guides + td, 4), "rmse": rmse(img)}
            rows[str(spp)] = row
        out["spp"] = rows
        target = out["fixed_1024"]["rmse"]
        ok = [(v["denoised_%s" % s]["wall_s"], "%s spp, %s" % (k, s)) for k, v in rows.items() for s in ("stats", "spatial")
              if v["denoised_%s" % s]["rmse"] <= target]
        out["headline"] = {"fixed_1024_rmse": target, "fixed_1024_wall_s": out["fixed_1024"]["wall_s"],
                           "fastest_denoised_at_or_below_that_rmse": min(ok)[1] if ok else None, "its_wall_s": min(ok)[0] if ok else None}
        doc[variant] = out
        r.close()
        print(json.dumps({variant: out}), file=sys.stderr, flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scenes", default="cornell_diffuse,cornell_roughdiel")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--spp", default="4,16,64,256")
    ap.add_argument("--phase", default="all", choices=["all", "quality", "kernels"])
    ap.add_argument("--rocprof-timeout", type=int, default=600)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
    W, H = a.width, a.height
    if a.phase == "kernels":
        kernels_phase(prt, W, H)
        return
    doc = {"width": W, "height": H, "ref_spp": a.ref_spp, "guide_spp": 4, "build_id": prt.build_id(),
           "filter": dict(prt.DENOISE_DEFAULTS)}
    doc["quality"] = quality(prt, a, W, H)
    if a.phase == "all":
        try:
            doc["kernel_time"] = kernel_times(W, H, a.rocprof_timeout)
        except (subprocess.SubprocessError, AssertionError, KeyError, OSError) as e:
            doc["kernel_time"] = {"error": repr(e)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
