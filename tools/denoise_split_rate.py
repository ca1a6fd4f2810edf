#!/usr/bin/env python3
"""What denoising from records costs beside prt_denoise, on the MI355X: prt_export_denoise_inputs and prt_denoise_records (5 passes) on the
records of a whole frame, against prt_denoise of the same context in the same run.  cornell (BASELINE config 2's scene) at 1920x1080,
16 spp rendered adaptively (min_spp = max_spp = 16, rel_err = 0: the picture plus its stats plane), guides at K = 4.
Wall time: REPS calls each, host clock around the call (every call is complete on return; the filter calls with no host output: prt_denoise
with both pointers NULL, prt_denoise_records into device memory).  Kernel time: the sum of the kernel durations of one call (best of REPS),
from `rocprofv3 --kernel-trace --stats` in a run of its own (this script with --phase kernels).  The outputs are compared as words first.
One JSON document on stdout (and into --out).

    python tools/denoise_split_rate.py [--width 1920 --height 1080] [--out profiles/r10_denoise_split.json]
"""
import argparse
import ctypes as C
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

SCENE = "cornell_diffuse.json"
SPP, GUIDE_K, PASSES, REPS = 16, 4, 5, 5


def _context(prt, W, H):
    scene = prt.HostScene(SCENE)
    r = prt.Renderer(scene.config(), device=0)
    r.upload_scene(scene)
    r.set_camera(prt.default_camera(W, H))
    r.resize(W, H)
    r.reset()
    r.render_adaptive(prt.seed_pairs(SPP * 64 + 64), SPP, SPP, 0.0)
    r.render_guides(GUIDE_K)
    return r


def _calls(prt, torch, r, W, H):
    """the three calls as closures over one set of buffers: export, prt_denoise (no output), prt_denoise_records (device output)"""
    records = torch.zeros((H, W, 16), dtype=torch.float32, device="cuda:0")
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    p = prt.DenoiseParams(PASSES, 1, 3.0, 128.0, 1.0, 0.1)             # PRT_DENOISE_VAR_STATS

    def export():
        r.export_denoise_inputs(records)

    def denoise():
        r._chk(r.lib.prt_denoise(r.ctx, C.byref(p), None, None), "prt_denoise")

    def denoise_records():
        r.denoise_records(records, W, H, passes=PASSES, var_source="stats", out=out)
    return records, out, export, denoise, denoise_records


def kernels_phase(prt, W, H):
    """the launches rocprofv3 times, in a fixed order: REPS x export, REPS x prt_denoise, REPS x prt_denoise_records"""
    import torch
    r = _context(prt, W, H)
    _, _, export, denoise, denoise_records = _calls(prt, torch, r, W, H)
    for fn in (export, denoise, denoise_records):
        for _ in range(REPS):
            fn()
    r.close()


def kernel_times(W, H, timeout):
    rows, stat_rows = kernel_rows(["--phase", "kernels", "--width", str(W), "--height", str(H)], "split", timeout, with_stats=True)
    rows = [(name, e - b) for name, b, e in rows]
    stat_rows = [row for row in stat_rows if "rec_" in row.get("Name", "") or "dn_" in row.get("Name", "")]
    mine = [(name, ns) for name, ns in rows if "rec_" in name or "dn_" in name]
    per_filter = 1 + 2 * PASSES                      # dn_var or rec_import, then (gauss, a-trous) per pass
    assert len(mine) == REPS * (1 + 2 * per_filter), len(mine)
    exports = mine[:REPS]
    den = [mine[REPS + k * per_filter:REPS + (k + 1) * per_filter] for k in range(REPS)]
    rec = [mine[REPS + (REPS + k) * per_filter:REPS + (REPS + k + 1) * per_filter] for k in range(REPS)]
    assert all("rec_export" in n for n, _ in exports) and all("dn_var" in c[0][0] for c in den) and all("rec_import" in c[0][0] for c in rec)

    def parts(call):
        return {"first_kernel": round(call[0][1] / 1e6, 4), "gauss_total": round(sum(ns for n, ns in call if "gauss" in n) / 1e6, 4),
                "atrous_per_pass": [round(ns / 1e6, 4) for n, ns in call if "atrous" in n]}
    best_den = min(den, key=lambda c: sum(ns for _, ns in c))
    best_rec = min(rec, key=lambda c: sum(ns for _, ns in c))
    return {"export_ms": round(min(ns for _, ns in exports) / 1e6, 4),
            "prt_denoise_ms": round(sum(ns for _, ns in best_den) / 1e6, 4), "prt_denoise_parts_ms": parts(best_den),
            "prt_denoise_records_ms": round(sum(ns for _, ns in best_rec) / 1e6, 4), "prt_denoise_records_parts_ms": parts(best_rec),
            "rocprofv3_stats": stat_rows,
            "note": "sum of the kernel durations of one call (best of %d) from rocprofv3 --kernel-trace --stats; first_kernel: dn_var_kernel "
                    "(prt_denoise) or rec_import_kernel (prt_denoise_records)" % REPS}


def wall_times(prt, W, H):
    import torch
    r = _context(prt, W, H)
    records, out, export, denoise, denoise_records = _calls(prt, torch, r, W, H)
    export()
    denoise_records()
    want = r.denoise(passes=PASSES, var_source="stats")
    same = bool((out.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all())
    doc = {"records_equal_prt_denoise_as_words": same}
    for name, fn in (("export", export), ("prt_denoise", denoise), ("prt_denoise_records", denoise_records)):
        fn()
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        doc[name + "_wall_ms"] = {"min": round(min(ts), 4), "median": round(float(np.median(ts)), 4)}
    r.close()
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--phase", default="all", choices=["all", "wall", "kernels"])
    ap.add_argument("--rocprof-timeout", type=int, default=300)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    prt = importlib.import_module("photorealistic-rendering-using-opencl_amd")
    W, H = a.width, a.height
    if a.phase == "kernels":
        kernels_phase(prt, W, H)
        return
    doc = {"width": W, "height": H, "scene": SCENE, "spp": SPP, "guide_spp": GUIDE_K, "passes": PASSES, "var_source": "stats",
           "build_id": prt.build_id(), "record_bytes_per_pixel": 64}
    doc["wall"] = wall_times(prt, W, H)
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
