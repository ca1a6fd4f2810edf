#!/usr/bin/env python3
"""What the temporal response (prt_set_temporal_response) costs in prt_denoise_temporal, on the MI355X.

Arms: the setting off and on (--on FASTCAP,RADIUS,K) in this tree and, with --parent-root DIR (a checkout of the parent commit with its
library built), the parent.  Each arm is a process of its own: cornell_diffuse at --width x --height, 4 spp and guides once, then --calls
prt_denoise_temporal calls (defaults, no read-back) timed one by one on the host.  The arms alternate, --rounds times; per arm the median and
the minimum of every round.  Kernel time: the durations of the reprojection (both instances), tm_clamp_kernel per radius and the a-trous
passes of the same calls, from `rocprofv3 --kernel-trace --stats` in a run of its own.  One JSON document on stdout (and into --out).

    python tools/response_rate.py [--parent-root DIR] [--out profiles/r26_response.json]

--doors: the same scheme over every filtering door instead -- prt_denoise, prt_denoise_temporal with the response off and on,
prt_denoise_records and prt_denoise_records_temporal (records of the same frame, output into device memory): per door and checkout the
pooled calls' median and quartiles, and the kernel names one call of each door launches, in order, from one kernel trace per checkout.

    python tools/response_rate.py --doors --parent-root DIR
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
PKG_NAME = "photorealistic-rendering-using-opencl_amd"
KERNEL_CALLS = 6
SETTINGS = ["off", "4,1,2", "4,2,2", "4,3,2"]


def _frame(root, W, H):
    sys.path.insert(0, root)
    prt = importlib.import_module(PKG_NAME)
    scene = prt.HostScene("cornell_diffuse.json")
    cfg = scene.config()
    r = prt.Renderer(cfg, device=0)
    r.upload_scene(scene)
    r.resize(W, H)
    r.set_camera(prt.default_camera(W, H))
    r.reset()
    r.render_spp(4, prt.seed_pairs(4 * max(cfg.max_bounces, 8) + 64))
    r.render_guides(4)
    return prt, r


def _set(r, response):
    if response == "off":
        if hasattr(r, "set_temporal_response"):
            r.set_temporal_response(None)
    else:
        f, rad, k = response.split(",")
        r.set_temporal_response(int(f), int(rad), float(k))


def _call(r):
    rc = r.lib.prt_denoise_temporal(r.ctx, None, None, None, None)
    assert rc == 0, rc


# --doors: label -> (door, the response setting it runs under; None: --on)
DOORS = {"prt_denoise": ("denoise", "off"), "prt_denoise_temporal, off": ("temporal", "off"), "prt_denoise_temporal, on": ("temporal", None),
         "prt_denoise_records": ("records", "off"), "prt_denoise_records_temporal": ("records_temporal", "off")}


def _door(prt, r, door, W, H):
    """one call of a door on r's frame as a closure: default parameters, no host output (the record doors write device memory)"""
    import ctypes as C
    lib, keep = r.lib, ()
    if door == "temporal":
        return lambda: _call(r)
    if door == "denoise":
        def fn():
            return lib.prt_denoise(r.ctx, None, None, None)
    else:
        import torch
        records = torch.zeros((H, W, 16), dtype=torch.float32, device="cuda:0")
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        r.export_denoise_inputs(records)
        rec, dst, cam = C.c_void_p(records.data_ptr()), C.c_void_p(out.data_ptr()), prt.default_camera(W, H)
        keep = (records, out)

        def fn():
            if door == "records":
                return lib.prt_denoise_records(r.ctx, None, W, H, rec, dst, None, None)
            return lib.prt_denoise_records_temporal(r.ctx, None, None, C.byref(cam), W, H, rec, dst, None, None)

    def call(keep=keep):                                                 # (the tensors live as long as the closure)
        rc = fn()
        assert rc == 0, rc
    return call


def arm_phase(a):
    prt, r = _frame(a.root, a.width, a.height)
    _set(r, a.response)
    call = _door(prt, r, a.door, a.width, a.height)
    for _ in range(4):
        call()
    ms = []
    for _ in range(a.calls):
        r.synchronize()
        t = time.perf_counter()
        call()                                                           # (complete on return: the call ends with a stream synchronise)
        ms.append(1e3 * (time.perf_counter() - t))
    r.close()
    print(json.dumps({"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "ms": [round(x, 4) for x in ms]}))


def sequence_phase(a):
    """one call of every door, each behind a one-sample guide render: the guide kernel marks where a door's launches begin in the trace"""
    prt, r = _frame(a.root, a.width, a.height)
    calls = [(response or a.on, _door(prt, r, door, a.width, a.height)) for door, response in DOORS.values()]     # (the exports run here)
    for response, call in calls:
        _set(r, response)
        r.render_guides(1)
        call()
    r.render_guides(1)
    r.close()


def door_sequences(a, root):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from _trace import kernel_rows
    rows = kernel_rows(["--phase", "sequence", "--root", root, "--on", a.on, "--width", str(a.width), "--height", str(a.height)], "doors", a.timeout)
    names = [name.split("(")[0].replace("prt::", "").replace("void ", "") for name, _, _ in rows]
    marks = [i for i, n in enumerate(names) if "guide" in n][-(len(DOORS) + 1):]
    return {label: names[b + 1:e] for label, b, e in zip(DOORS, marks[:-1], marks[1:])}


def doors_main(a):
    roots = [("tree", ROOT)] + ([("parent", os.path.abspath(a.parent_root))] if a.parent_root else [])
    doc = {"frame": [a.width, a.height], "calls_per_round": a.calls, "rounds": a.rounds, "wall ms per call (host clock; every call ends with a stream synchronise)": {},
           "kernels of one call, in launch order": {}}
    for label, (door, response) in DOORS.items():
        ms = {name: [] for name, _ in roots}
        for _ in range(a.rounds):
            for name, root in reversed(roots):
                cmd = [sys.executable, os.path.abspath(__file__), "--phase", "arm", "--root", root, "--door", door, "--response", response or a.on,
                       "--width", str(a.width), "--height", str(a.height), "--calls", str(a.calls)]
                p = subprocess.run(cmd, check=True, timeout=a.timeout, capture_output=True, text=True)
                ms[name] += json.loads(p.stdout.strip().splitlines()[-1])["ms"]
        doc["wall ms per call (host clock; every call ends with a stream synchronise)"][label] = {
            name: dict(zip(("q25", "median", "q75"), (round(float(q), 4) for q in np.percentile(v, (25, 50, 75))))) for name, v in ms.items()}
    for name, root in roots:
        doc["kernels of one call, in launch order"][name] = door_sequences(a, root)
    if a.parent_root:
        seq = doc["kernels of one call, in launch order"]
        doc["launch sequences equal the parent's"] = seq["tree"] == seq["parent"]
    return doc


def kernels_phase(a):
    prt, r = _frame(a.root, a.width, a.height)
    for s in SETTINGS:
        _set(r, s)
        for _ in range(KERNEL_CALLS):
            _call(r)
    r.close()


def kernel_times(a, root=ROOT):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from _trace import kernel_rows
    rows, stats = kernel_rows(["--phase", "kernels", "--root", root, "--width", str(a.width), "--height", str(a.height)], "resp", a.timeout, with_stats=True)
    per = {}
    for name, b, e in rows:
        if "tm_" in name or "dn_" in name:
            key = name.split("(")[0].replace("prt::", "").replace("void ", "")
            per.setdefault(key, []).append(e - b)
    out = {k: {"calls": len(v), "median_us": round(float(np.median(v)) / 1e3, 2), "min_us": round(min(v) / 1e3, 2)} for k, v in sorted(per.items())}
    # the a-trous launches by pass (step 2^i): five per call, in order
    atrous = [e - b for name, b, e in rows if "dn_atrous" in name]
    by_pass = [atrous[i::5] for i in range(5)]
    out["dn_atrous_kernel by pass, median_us"] = [round(float(np.median(p)) / 1e3, 2) for p in by_pass]
    return {"kernels": out, "rocprofv3_stats": [s for s in stats if "tm_" in s.get("Name", "") or "dn_" in s.get("Name", "")],
            "note": "%d calls per setting (%s), still camera, history valid from each setting's second call" % (KERNEL_CALLS, " | ".join(SETTINGS))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", default="all", choices=["all", "arm", "kernels", "sequence"])
    ap.add_argument("--doors", action="store_true", help="every filtering door instead of the response's cost")
    ap.add_argument("--door", default="temporal", choices=["denoise", "temporal", "records", "records_temporal"], help="(arm phase) the call timed")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--response", default="off")
    ap.add_argument("--on", default="4,2,2", help="the setting of the 'on' arm")
    ap.add_argument("--root", default=ROOT, help="(arm phase) the checkout whose package and library the arm runs")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--variant-root", default=None, help="a checkout with an experimental library: one more 'on' arm and its kernel times")
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.phase == "arm":
        return arm_phase(a)
    if a.phase == "kernels":
        return kernels_phase(a)
    if a.phase == "sequence":
        return sequence_phase(a)
    if a.doors:
        text = json.dumps(doors_main(a), indent=1)
        print(text)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(text + "\n")
        return
    arms = [("tree, off", ROOT, "off"), ("tree, on (%s)" % a.on, ROOT, a.on)]
    if a.parent_root:
        arms.insert(0, ("parent, off", os.path.abspath(a.parent_root), "off"))
    if a.variant_root:
        arms.append(("variant, on (%s)" % a.on, os.path.abspath(a.variant_root), a.on))
    res = {name: [] for name, _, _ in arms}
    for _ in range(a.rounds):
        for name, root, response in arms:
            cmd = [sys.executable, os.path.abspath(__file__), "--phase", "arm", "--root", root, "--response", response, "--width", str(a.width),
                   "--height", str(a.height), "--calls", str(a.calls)]
            p = subprocess.run(cmd, check=True, timeout=a.timeout, capture_output=True, text=True)
            res[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    doc = {"frame": [a.width, a.height], "calls_per_round": a.calls,
           "prt_denoise_temporal wall ms per round (host clock around the call, which ends with a stream synchronise)": res,
           "median of the rounds' medians": {k: round(float(np.median([x["median_ms"] for x in v])), 4) for k, v in res.items()},
           "spread of the rounds' medians (max - min)": {k: round(max(x["median_ms"] for x in v) - min(x["median_ms"] for x in v), 4) for k, v in res.items()}}
    doc.update(kernel_times(a))
    if a.variant_root:
        doc["variant"] = kernel_times(a, os.path.abspath(a.variant_root))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
