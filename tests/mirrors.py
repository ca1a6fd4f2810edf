"""tests/mirrors.py -- TEST INFRASTRUCTURE: the yardsticks.  Numpy restatements of the rules written down in include/prt.h (and, for the known
answers, of the OpenCL specification), which share no code with the product or with the emulators under tests/emu: what the library, the
bodies run on the host and the device are measured against.  A plain module (no fixtures, no hooks, no test); it imports no test module
and nothing from tests/cases.py.  The one thing taken from the package is the byte layout of the reference's BVH node (NODE_T), which is
data of the ABI, not code.

A mirror is edited only when prt.h changes: every test file that names it is measured against the same text."""
import ctypes as C
import math
import os

import numpy as np

from conftest import GOLDEN
from support import pkg as _pkg

f32 = np.float32
NODE_T = np.dtype(_pkg()._capi.BVH_NODE_DTYPE)


# ---- the tree: prt.h's box rules (prt_update_vertices) and rules 1 - 8 of prt_rebuild_bvh --------------------------------------------------------

def mirror_refit(nodes, primitive_indices, vertices):
    """the nodes refitted by the rules of prt.h: leaf boxes from the vertices in leaf order (vertices 0, 1, 2 of each triangle), inner boxes
    = child 0's with child 1's merged, children before parents; an empty leaf and a node the root does not reach keep their boxes"""
    out = nodes.copy()
    v = np.ascontiguousarray(vertices, dtype=f32).reshape(-1, 4)
    order, stack = [], [0]
    while stack:
        n = stack.pop()
        order.append(n)
        if not out[n]["leaf"]:
            stack += [int(out[n]["first"]), int(out[n]["first"]) + 1]
    for n in reversed(order):                    # reversed pre-order: every child before its parent
        first, count = int(out[n]["first"]), int(out[n]["count"])
        if out[n]["leaf"]:
            if count == 0:
                continue
            fv = primitive_indices[first:first + count].astype(np.uint32) * np.uint32(3)
            pts = v[(fv[:, None] + np.arange(3, dtype=np.uint32)[None, :]).reshape(-1), :3]
            lo, hi = pts[0].copy(), pts[0].copy()
            for c in pts[1:]:
                lo = np.where(c < lo, c, lo)
                hi = np.where(c > hi, c, hi)
        else:
            b0, b1 = out[first]["bounds"], out[first + 1]["bounds"]
            lo, hi = b0[0::2].copy(), b0[1::2].copy()
            lo = np.where(b1[0::2] < lo, b1[0::2], lo)
            hi = np.where(b1[1::2] > hi, b1[1::2], hi)
        out[n]["bounds"][0::2] = lo
        out[n]["bounds"][1::2] = hi
    return out


DEFAULT_LEAF = 4                # what max_leaf = 0 stands for (prt.h)


def mirror_keys(vertices):
    """rules 1 - 4: the sorted keys as Python ints"""
    v = np.ascontiguousarray(vertices, dtype=f32).reshape(-1, 3, 4)[:, :, :3]
    lo, hi = v[:, 0].copy(), v[:, 0].copy()
    for k in (1, 2):
        lo = np.where(v[:, k] < lo, v[:, k], lo)
        hi = np.where(v[:, k] > hi, v[:, k], hi)
    c = lo * f32(0.5) + hi * f32(0.5)
    assert c.dtype == f32
    elo, ehi = c.min(0) + f32(0.0), c.max(0) + f32(0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(ehi > elo, f32(1024.0) / (ehi - elo), f32(0.0)).astype(f32)
    t = (c - elo) * scale
    assert t.dtype == f32
    q = np.where(t < f32(1023.0), t, f32(1023.0)).astype(np.uint32)
    keys = []
    for i in range(len(v)):
        code = 0
        for bit in range(10):
            for axis in range(3):                  # x in the highest bit of each triple, then y, then z
                code |= ((int(q[i, axis]) >> bit) & 1) << (3 * bit + 2 - axis)
        keys.append((code << 32) | i)
    return sorted(keys), q


_built = {}


def mirror_build(vertices, max_leaf):
    """rules 1 - 8: (nodes, primitive_indices, levels of pairs, stack_levels); computed once per input, shared, never written to"""
    key = (hash(np.ascontiguousarray(vertices, dtype=f32).tobytes()), int(max_leaf))
    if key not in _built:
        _built[key] = _mirror_build(vertices, max_leaf)
        for a in _built[key][:2]:
            a.setflags(write=False)
    return _built[key]


def _mirror_build(vertices, max_leaf):
    keys, _ = mirror_keys(vertices)
    T = len(keys)
    assert len(set(keys)) == T
    prims = np.zeros(T, dtype=np.uint64)
    if T <= max_leaf:
        nodes = np.zeros(1, dtype=NODE_T)
        nodes[0]["count"], nodes[0]["leaf"] = T, 1
        prims[:] = [k & 0xFFFFFFFF for k in keys]
        return mirror_refit(nodes, prims, vertices), prims, 0, 1
    queue = [(0, T - 1, 0, 0)]                     # inner ranges in breadth-first order: (a, b, depth, pairs with two inner children above)
    recs, slot, head, deepest, most_two = [], 0, 0, 0, 0
    while head < len(queue):
        a, b, depth, two_above = queue[head]
        head += 1
        bit = (keys[a] ^ keys[b]).bit_length() - 1
        lo_, hi_ = a, b                            # the largest g in [a, b) whose key has a 0 in `bit`: the keys are sorted
        while lo_ < hi_:
            mid = (lo_ + hi_ + 1) // 2
            if (keys[mid] >> bit) & 1:
                hi_ = mid - 1
            else:
                lo_ = mid
        g = lo_
        assert a <= g < b and not (keys[g] >> bit) & 1 and (keys[g + 1] >> bit) & 1
        kids = [(a, g), (g + 1, b)]
        inner = [y - x + 1 > max_leaf for x, y in kids]
        two = two_above + (1 if all(inner) else 0)
        most_two, deepest = max(most_two, two), max(deepest, depth)
        rec = []
        for (x, y), is_inner in zip(kids, inner):
            if is_inner:
                rec.append((0, 2 * len(queue) + 1, 0))
                queue.append((x, y, depth + 1, two))
            else:
                rec.append((1, slot, y - x + 1))
                prims[slot:slot + y - x + 1] = [k & 0xFFFFFFFF for k in keys[x:y + 1]]
                slot += y - x + 1
        recs.append(rec)
    assert slot == T
    nodes = np.zeros(2 * len(recs) + 1, dtype=NODE_T)
    nodes[0]["first"] = 1
    for k, rec in enumerate(recs):
        for ch, (leaf, first, count) in enumerate(rec):
            nodes[2 * k + 1 + ch]["leaf"], nodes[2 * k + 1 + ch]["first"], nodes[2 * k + 1 + ch]["count"] = leaf, first, count
    return mirror_refit(nodes, prims, vertices), prims, deepest + 1, most_two + 1


# ---- smooth normals (prt_set_smooth_normals), float32 --------------------------------------------------------------------------------------------

UNIT, AREA = 0, 1
LOADER_CREASE_COS = -0.99619470


def mirror_weld(vertices):
    """groups by bit-identical position after x + 0.0f, numbered by first appearance in corner order"""
    key = (np.ascontiguousarray(vertices, dtype=f32).reshape(-1, 4)[:, :3] + f32(0.0)).copy().view(np.uint32)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)].astype(np.uint32), len(first)


def mirror_faces(vertices):
    """(r, l, f) of prt.h per face, float32"""
    v = np.ascontiguousarray(vertices, dtype=f32).reshape(-1, 3, 4)
    a, b, c = v[:, 0, :3], v[:, 1, :3], v[:, 2, :3]
    with np.errstate(all="ignore"):
        u, w = b - a, c - a
        r = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        l = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        f = np.where((l > 0)[:, None], r / l[:, None], r)
    assert r.dtype == f32 and l.dtype == f32 and f.dtype == f32
    return r, l, f


def mirror_normals(vertices, groups, weighting=UNIT, crease_cos=LOADER_CREASE_COS):
    """float32 [3T, 4]: the corner rule of prt.h; step k adds member k of every corner's group, so every sum runs in member order"""
    r, l, f = mirror_faces(vertices)
    g = np.asarray(groups, dtype=np.int64)
    n = len(g)
    order = np.argsort(g, kind="stable")                       # corners by group, ascending corner index within a group
    count = np.bincount(g, minlength=int(g.max()) + 1)
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    fi = f[np.arange(n) // 3]
    s = np.zeros((n, 3), dtype=f32)
    crease = f32(crease_cos)
    with np.errstate(all="ignore"):
        for k in range(int(count.max())):
            act = np.nonzero(count[g] > k)[0]
            j = order[first[g[act]] + k] // 3
            fj, me = f[j], fi[act]
            d = (fj[:, 0] * me[:, 0] + fj[:, 1] * me[:, 1]) + fj[:, 2] * me[:, 2]
            ok = d >= crease                                   # (False for a NaN d)
            add = fj if weighting == UNIT else r[j]
            s[act] = np.where(ok[:, None], s[act] + add, s[act])
        L = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        out = np.zeros((n, 4), dtype=f32)
        out[:, :3] = np.where((L > 0)[:, None], s / L[:, None], fi)
    assert s.dtype == f32 and L.dtype == f32
    return out


# ---- the deformers (prt_pose, prt_morph), float32 ------------------------------------------------------------------------------------------------

def mirror_pose(rest_v, rest_n, index, weight, matrices):
    """(vertices, normals) float32 [n, 4] by the formulas of prt.h; normals None without rest normals"""
    v = np.ascontiguousarray(rest_v, dtype=f32).reshape(-1, 4)
    idx = np.ascontiguousarray(index, dtype=np.uint16).reshape(-1, 4).astype(np.int64)
    w = np.ascontiguousarray(weight, dtype=f32).reshape(-1, 4)
    M = np.ascontiguousarray(matrices, dtype=f32).reshape(-1, 3, 4)
    n = len(v)
    A = np.zeros((n, 3, 4), dtype=f32)
    with np.errstate(all="ignore"):
        for k in range(4):
            wk = w[:, k][:, None, None]
            A = A + np.where(wk != 0, wk * M[idx[:, k]], f32(0))
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        out_v = np.zeros((n, 4), dtype=f32)
        for i in range(3):
            out_v[:, i] = ((A[:, i, 0] * x + A[:, i, 1] * y) + A[:, i, 2] * z) + A[:, i, 3]
        assert A.dtype == f32
        if rest_n is None:
            return out_v, None
        r = np.ascontiguousarray(rest_n, dtype=f32).reshape(-1, 4)
        nx, ny, nz = r[:, 0], r[:, 1], r[:, 2]
        q = np.stack([(A[:, i, 0] * nx + A[:, i, 1] * ny) + A[:, i, 2] * nz for i in range(3)], axis=1)
        L = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
        out_n = np.zeros((n, 4), dtype=f32)
        out_n[:, :3] = np.where((L > 0)[:, None], q / L[:, None], q)
        assert q.dtype == f32 and L.dtype == f32
    return out_v, out_n


def mirror_morph_raw(base_v, base_n, targets, weights):
    """(p, n) float32 [corners, 4], un-normalised, lane 3 the base's; n None without base normals"""
    p = np.array(base_v, dtype=f32).reshape(-1, 4)
    n = None if base_n is None else np.array(base_n, dtype=f32).reshape(-1, 4)
    w = np.asarray(weights, dtype=f32).reshape(-1)
    assert len(w) == len(targets)
    with np.errstate(all="ignore"):
        for t, (corner, dp, dn) in enumerate(targets):
            if w[t] == 0 or len(corner) == 0:
                continue
            corner = np.asarray(corner, dtype=np.int64)
            p[corner, :3] = p[corner, :3] + w[t] * np.asarray(dp, dtype=f32).reshape(-1, 4)[:, :3]
            if n is not None:
                delta = np.zeros((len(corner), 3), dtype=f32) if dn is None else np.asarray(dn, dtype=f32).reshape(-1, 4)[:, :3]
                n[corner, :3] = n[corner, :3] + w[t] * delta
    assert p.dtype == f32 and (n is None or n.dtype == f32)
    return p, n


def mirror_morph(base_v, base_n, targets, weights):
    """(vertices, normals) float32 [corners, 4] of prt_morph by the formulas of prt.h; normals None without base normals"""
    p, n = mirror_morph_raw(base_v, base_n, targets, weights)
    out_v = np.zeros_like(p)
    out_v[:, :3] = p[:, :3]
    if n is None:
        return out_v, None
    with np.errstate(all="ignore"):
        x, y, z = n[:, 0], n[:, 1], n[:, 2]
        L = np.sqrt((x * x + y * y) + z * z)
        out_n = np.zeros_like(n)
        out_n[:, :3] = np.where((L > 0)[:, None], n[:, :3] / L[:, None], n[:, :3])
        assert L.dtype == f32
    return out_v, out_n


# ---- the pixel filter (prt_set_pixel_filter, prt_pixel_filter_offsets) ---------------------------------------------------------------------------

KINDS = {"box": 1, "tent": 2, "gaussian": 3, "blackman-harris": 4}
DEFAULT_R = {"box": 0.5, "tent": 1.0, "gaussian": 1.5, "blackman-harris": 2.0}
BH = (0.35875, 0.48829, 0.14128, 0.01168)
SETS = [("cornell_diffuse.json", False, "LIGHT|DIFF"), ("cornell_coat.json", False, "COAT"), ("cornell_roughcond.json", True, "ROUGH_COND"),
        ("cornell_roughdiel.json", True, "ROUGH_DIEL"), ("cornell_diffuse.json", False, "generic"), ("cornell_media.json", True, "medium"),
        ("cornell_mixed.json", True, "generic")]


def lowbias32(v):
    v = np.asarray(v, dtype=np.uint32)
    with np.errstate(over="ignore"):
        v = v ^ (v >> np.uint32(16)); v = v * np.uint32(0x7FEB352D)
        v = v ^ (v >> np.uint32(15)); v = v * np.uint32(0x846CA68B)
        return v ^ (v >> np.uint32(16))


def sample_u(gx, gy, k):
    """(u, v) of paths k (uint32 array) of global pixel (gx, gy): float32, exact"""
    k = np.asarray(k, dtype=np.uint32)
    with np.errstate(over="ignore"):
        s = np.uint32(gy) * np.uint32(0x9E3779B9) + np.uint32(gx)
        ux = k * np.uint32(3242174889) + lowbias32(s)
        uy = k * np.uint32(2447445414) + lowbias32(s ^ np.uint32(0x68E31DA4))
    f = lambda x: (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return f(ux), f(uy)


def marginal_cdf(kind, x, r):
    """the normalised CDF of the kind's 1-D profile on [-r, r], float64, closed form"""
    x = np.clip(np.asarray(x, dtype=np.float64), -r, r)
    if kind == "box":
        return (x + r) / (2 * r)
    if kind == "tent":
        return np.where(x < 0, (x + r) ** 2 / (2 * r * r), 1 - (r - x) ** 2 / (2 * r * r))
    if kind == "gaussian":
        s = r / 3.0
        c = math.exp(-r * r / (2 * s * s))
        erf = np.vectorize(math.erf)
        G = lambda t: s * math.sqrt(math.pi / 2) * erf(t / (s * math.sqrt(2))) - c * t
    else:
        a0, a1, a2, a3 = BH
        G = lambda t: (a0 * t + a1 * r / math.pi * np.sin(math.pi * t / r) + a2 * r / (2 * math.pi) * np.sin(2 * math.pi * t / r)
                       + a3 * r / (3 * math.pi) * np.sin(3 * math.pi * t / r))
    return (G(x) - G(-r)) / (G(r) - G(-r))


def table(kind, r):
    """T[0 .. 256] of prt.h: F^-1(i / 256) by bisection in float64, rounded to float32, antisymmetric"""
    T = np.zeros(257, dtype=np.float64)
    if r > 0:
        p = np.arange(1, 128) / 256.0
        lo, hi = np.full(127, -float(r)), np.zeros(127)
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            below = marginal_cdf(kind, mid, r) < p
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        T[1:128] = 0.5 * (lo + hi)
        T[0] = -r
    T[129:] = -T[127::-1]
    T[128] = 0.0
    return T.astype(np.float32)


def warp(kind, r, u, T=None):
    f = np.float32
    u = np.asarray(u, dtype=f)
    r = f(r)
    if kind == "box":
        return (u - f(0.5)) * (f(2) * r)
    if kind == "tent":
        with np.errstate(invalid="ignore"):
            lo = r * (np.sqrt(f(2) * u) - f(1))
            hi = r * (f(1) - np.sqrt(f(2) - f(2) * u))
        return np.where(u < f(0.5), lo, hi).astype(f)
    t = u * f(256)
    j = np.minimum(t.astype(np.int64), 255)
    t = t - j.astype(f)
    return (T[j] + t * (T[j + 1] - T[j])).astype(f)


def offsets_ref(kind, r, gx, gy, k0, n):
    k = (np.uint64(k0) + np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    u, v = sample_u(gx, gy, k.astype(np.uint32))
    T = table(kind, r) if kind in ("gaussian", "blackman-harris") else None
    return np.stack([warp(kind, r, u, T), warp(kind, r, v, T)], -1)


# ---- the a-trous filter in float64 (prt_denoise) -------------------------------------------------------------------------------------------------

def lum(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def stats_variance(l, s2, n):
    """v of PRT_DENOISE_VAR_STATS, in float32 with the device's operations (the difference cancels: float64 would not be the same input)"""
    f = np.float32
    l, s2 = np.asarray(l, dtype=f), np.asarray(s2, dtype=f)
    n = np.asarray(n, dtype=np.uint32)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = l / n.astype(f)
        v = np.maximum((s2 - l * m) / (n.astype(f) * (n - np.uint32(1)).astype(f)), f(0))
    return np.where(n >= 2, v, f(0)).astype(np.float64)


def _clamped(a, dy, dx):
    H, W = a.shape[:2]
    ys = np.clip(np.arange(H) + dy, 0, H - 1)
    xs = np.clip(np.arange(W) + dx, 0, W - 1)
    return a[ys][:, xs]


def spatial_variance(rgb):
    L = lum(rgb)
    fin = np.isfinite(rgb).all(-1)
    s1 = np.zeros(L.shape); s2 = np.zeros(L.shape); cnt = np.zeros(L.shape)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            l, f = _clamped(L, dy, dx), _clamped(fin, dy, dx)
            s1 += np.where(f, l, 0); s2 += np.where(f, l * l, 0); cnt += f
    with np.errstate(divide="ignore", invalid="ignore"):
        m = s1 / cnt
        return np.where(cnt > 0, np.maximum(s2 / cnt - m * m, 0.0), 0.0)


def _grad(z, cov):
    H, W = z.shape
    g = np.zeros((H, W))
    for axis in (0, 1):
        def shift(a, d, fill):
            out = np.full_like(a, fill)
            if axis == 1:
                if d > 0: out[:, :-d] = a[:, d:]
                else: out[:, -d:] = a[:, :d]
            else:
                if d > 0: out[:-d] = a[d:]
                else: out[-d:] = a[:d]
            return out
        za, ha = shift(z, 1, 0.0), shift(cov > 0, 1, False)
        zb, hb = shift(z, -1, 0.0), shift(cov > 0, -1, False)
        d = np.where(ha & hb, 0.5 * np.abs(za - zb), np.where(ha, np.abs(za - z), np.where(hb, np.abs(z - zb), 0.0)))
        g = np.maximum(g, d)
    return np.where(cov > 0, g, 0.0)


def denoise_ref(fb, guides, v, passes=5, sigma_l=3.0, sigma_n=128.0, sigma_z=1.0, sigma_a=0.1):
    """prt.h's filter in float64: fb [H, W, 4], guides [H, W, 8], v [H, W] -> rgba [H, W, 4]"""
    old = np.seterr(all="ignore")
    fb = fb.astype(np.float64)
    g8 = guides.astype(np.float64)
    a, cov, n, z = g8[..., 0:3], g8[..., 3], g8[..., 4:7], g8[..., 7]
    H, W = fb.shape[:2]
    c, v = fb[..., :3].copy(), v.astype(np.float64).copy()
    own_fin = np.isfinite(fb[..., :3]).all(-1)
    grad = _grad(z, cov)
    k = {-2: 1 / 16, -1: 1 / 4, 0: 3 / 8, 1: 1 / 4, 2: 1 / 16}
    for i in range(passes):
        s = 1 << i
        gv = np.zeros((H, W))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                gv += (2 if dx == 0 else 1) * (2 if dy == 0 else 1) / 16 * _clamped(v, dy, dx)
        lp = lum(c)
        sw = np.zeros((H, W)); sc = np.zeros((H, W, 3)); sv = np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = np.arange(H)[:, None] + s * dy, np.arange(W)[None, :] + s * dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qyc, qxc = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                cq, vq = c[qyc, qxc], v[qyc, qxc]
                ok = inside & np.isfinite(cq).all(-1)
                cq = np.where(ok[..., None], cq, 0.0)
                covq, nq, zq, aq = cov[qyc, qxc], n[qyc, qxc], z[qyc, qxc], a[qyc, qxc]
                both = (cov > 0) & (covq > 0)
                wn = np.where(both, np.maximum(0.0, (n * nq).sum(-1)) ** sigma_n, np.where((cov > 0) == (covq > 0), 1.0, 0.0))
                wz = np.exp(-np.abs(z - zq) / (sigma_z * grad * s * np.sqrt(dx * dx + dy * dy) + 1e-4))
                wa = np.exp(-((a - aq) ** 2).sum(-1) / sigma_a ** 2)
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    wl = np.exp(-np.abs(lp - lum(cq)) / (sigma_l * np.sqrt(gv) + 1e-6))
                w = 1.0 if dx == 0 and dy == 0 else wn * wz * wa * wl           # the centre tap: w = 1
                ok = ok & (w > 0)                                                  # (a NaN weight drops the tap)
                hw = np.where(ok, k[dx] * k[dy] * w, 0.0)
                sw += hw; sc += hw[..., None] * cq; sv += hw * hw * np.where(ok, vq, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(own_fin[..., None], sc / sw[..., None], c)
            v = np.where(own_fin, sv / (sw * sw), v)
    np.seterr(**old)
    return np.concatenate([c, fb[..., 3:4]], -1)


# ---- temporal reprojection in float64 (prt_denoise_temporal, with and without a motion plane) ----------------------------------------------------

def _nrm(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def camera_basis(cam):
    """camera_basis (pt_device.h) in float64: P, M, Hz, Vt"""
    P, view, up = (np.array(x[:3], dtype=np.float64) for x in (cam.position, cam.view, cam.up))
    view, up = _nrm(view), _nrm(up)
    h = _nrm(np.cross(view, up))
    v = _nrm(np.cross(h, view))
    return P, P + view, h * np.tan(np.radians(cam.fov[0] * 0.5)), v * np.tan(np.radians(cam.fov[1] * -0.5))


def centre_dirs(B, W, H, xs=None, ys=None):
    """create_cam_ray's centre-ray direction of pixel (x, y) -- continuous coordinates allowed"""
    P, M, Hz, Vt = B
    if xs is None:
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    sx, sy = xs / (W - 1.0), (H - 1.0 - ys) / (H - 1.0)
    on = M + Hz * (2 * sx - 1)[..., None] + Vt * (2 * sy - 1)[..., None]
    return _nrm(on - P)


def project(B, e, W, H):
    """prt.h: e (X - P, or a direction) -> (x', y', dot(e, M - P))"""
    P, M, Hz, Vt = B
    f = M - P
    ef = e @ f
    with np.errstate(divide="ignore", invalid="ignore"):
        q = e * ((f @ f) / ef)[..., None] - f
    a, b = (q @ Hz) / (Hz @ Hz), (q @ Vt) / (Vt @ Vt)
    return (a + 1) / 2 * (W - 1), (H - 1) - (b + 1) / 2 * (H - 1), ef


def temporal_ref(fb, g, g_prev, hist_prev, cam, cam_prev, v_frame, alpha_color=0.2, alpha_moments=0.2, tau_z=0.05, cos_n=0.9,
                 history_cap=32):
    """prt.h's reprojection and accumulation in float64.  fb [H, W, 4], g / g_prev [H, W, 8] (guides now / at the previous call),
    hist_prev [H, W, 8] (None: empty history), v_frame [H, W] (prt_denoise's v of this frame).  Returns a dict of c_i [H, W, 3], n, m1,
    m2, v, hist (had history), margin (every decision of the pixel is clear of its threshold) and the per-pixel scales of the inputs
    blended (for relative comparisons).  For test_temporal_records.py, which checks the n >= 4 switch itself: margin_other (margin without
    the n = 4 term), near4 (|n - 4| <= 1e-3) and sw (the sum of the valid taps' weights)."""
    old = np.seterr(all="ignore")
    H, W = fb.shape[:2]
    c = fb[..., :3].astype(np.float64)
    L = lum(c)
    fin = np.isfinite(c).all(-1)
    g, g_prev = g.astype(np.float64), g_prev.astype(np.float64)
    cov, nrm, z = g[..., 3] > 0, g[..., 4:7], g[..., 7]
    B, Bp = camera_basis(cam), camera_basis(cam_prev)
    d = centre_dirs(B, W, H)
    e = np.where(cov[..., None], B[0] + d * z[..., None] - Bp[0], d)
    dist = np.where(cov, np.linalg.norm(e, axis=-1), 0.0)
    xp, yp, ef = project(Bp, e, W, H)
    f = Bp[1] - Bp[0]
    front = ef > 0
    margin = np.abs(ef) > 1e-6 * np.linalg.norm(e, axis=-1) * np.linalg.norm(f)
    inr = front & (xp > -1) & (xp < W) & (yp > -1) & (yp < H)
    grad = _grad(z, g[..., 3])
    x0, y0 = np.floor(np.where(inr, xp, 0)), np.floor(np.where(inr, yp, 0))
    fx, fy = np.where(inr, xp, 0) - x0, np.where(inr, yp, 0) - y0
    sw = np.zeros((H, W)); sc = np.zeros((H, W, 3)); sn = np.zeros((H, W)); s1 = np.zeros((H, W)); s2 = np.zeros((H, W))
    cmax = np.abs(c).max(-1); m1max = np.abs(L); m2max = L * L
    have = hist_prev is not None
    hp = hist_prev.astype(np.float64) if have else np.zeros((H, W, 8))
    for t in range(4):
        tx, ty = x0.astype(np.int64) + (t & 1), y0.astype(np.int64) + (t >> 1)
        w = (fx if t & 1 else 1 - fx) * (fy if t >> 1 else 1 - fy)
        inside = inr & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        txc, tyc = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
        h, gq = hp[tyc, txc], g_prev[tyc, txc]
        ok = inside & np.isfinite(h[..., :3]).all(-1) & ((gq[..., 3] > 0) == cov)
        dz = np.abs(gq[..., 7] - dist)
        tol = tau_z * dist + grad
        dn = (nrm * gq[..., 4:7]).sum(-1)
        ok_geo = ~cov | ((dz <= tol) & (dn >= cos_n))
        weighty = ok & (w > 1e-6) & cov
        margin &= ~weighty | ((np.abs(dz - tol) > 1e-4 * np.maximum(tol, 1e-6)) & (np.abs(dn - cos_n) > 1e-4))
        ok &= ok_geo
        wv = np.where(ok, w, 0.0)
        hv = np.where(ok[..., None], h, 0.0)
        sw += wv; sc += wv[..., None] * hv[..., :3]; sn += wv * hv[..., 3]; s1 += wv * hv[..., 4]; s2 += wv * hv[..., 5]
        big = ok & (w > 1e-6)
        cmax = np.maximum(cmax, np.where(big, np.abs(hv[..., :3]).max(-1), 0))
        m1max = np.maximum(m1max, np.where(big, np.abs(hv[..., 4]), 0))
        m2max = np.maximum(m2max, np.where(big, np.abs(hv[..., 5]), 0))
    hist = have & fin & inr & (sw >= 0.01)
    margin &= np.abs(sw - 0.01) > 1e-4
    inv = np.where(hist, 1.0 / np.where(sw > 0, sw, 1.0), 0.0)
    ch, nh, m1h, m2h = sc * inv[..., None], sn * inv, s1 * inv, s2 * inv
    n = np.where(hist, np.minimum(nh + 1, history_cap), 1.0)
    ac, am = np.maximum(alpha_color, 1 / n), np.maximum(alpha_moments, 1 / n)
    ci = np.where(hist[..., None], ch + ac[..., None] * (c - ch), c)
    m1 = np.where(hist, m1h + am * (L - m1h), L)
    m2 = np.where(hist, m2h + am * (L * L - m2h), L * L)
    margin_other = margin.copy()
    near4 = np.abs(n - 4) <= 1e-3
    margin &= ~near4
    v = np.where(n >= 4, np.maximum(m2 - m1 * m1, 0.0), v_frame)
    np.seterr(**old)
    return dict(ci=ci, n=n, m1=m1, m2=m2, v=v, hist=hist, margin=margin, cscale=cmax, m1scale=m1max, m2scale=m2max,
                margin_other=margin_other, near4=near4, sw=sw)


def _close(got, ref, scale, rel=1e-4):
    return np.abs(got - ref) <= rel * np.maximum(scale, 1e-6)


def temporal_ref_motion(fb, g, g_prev, hist_prev, cam, cam_prev, v_frame, motion=None, alpha_color=0.2, alpha_moments=0.2, tau_z=0.05,
                        cos_n=0.9, history_cap=32):
    """temporal_ref plus the motion plane: motion [H, W, 4] = {D, m} or None.  A covered pixel with m > 0 and D != 0 reprojects
    X + D; nothing else differs"""
    old = np.seterr(all="ignore")
    H, W = fb.shape[:2]
    c = fb[..., :3].astype(np.float64)
    L = lum(c)
    fin = np.isfinite(c).all(-1)
    g, g_prev = g.astype(np.float64), g_prev.astype(np.float64)
    cov, nrm, z = g[..., 3] > 0, g[..., 4:7], g[..., 7]
    B, Bp = camera_basis(cam), camera_basis(cam_prev)
    d = centre_dirs(B, W, H)
    X = B[0] + d * z[..., None]
    if motion is not None:
        mo = np.asarray(motion, dtype=np.float64)
        moved = cov & (mo[..., 3] > 0) & (mo[..., :3] != 0).any(-1)
        X = np.where(moved[..., None], X + mo[..., :3], X)
    e = np.where(cov[..., None], X - Bp[0], d)
    dist = np.where(cov, np.linalg.norm(e, axis=-1), 0.0)
    xp, yp, ef = project(Bp, e, W, H)
    f = Bp[1] - Bp[0]
    front = ef > 0
    margin = np.abs(ef) > 1e-6 * np.linalg.norm(e, axis=-1) * np.linalg.norm(f)
    inr = front & (xp > -1) & (xp < W) & (yp > -1) & (yp < H)
    grad = _grad(z, g[..., 3])
    x0, y0 = np.floor(np.where(inr, xp, 0)), np.floor(np.where(inr, yp, 0))
    fx, fy = np.where(inr, xp, 0) - x0, np.where(inr, yp, 0) - y0
    sw = np.zeros((H, W)); sc = np.zeros((H, W, 3)); sn = np.zeros((H, W)); s1 = np.zeros((H, W)); s2 = np.zeros((H, W))
    cmax = np.abs(c).max(-1); m1max = np.abs(L); m2max = L * L
    have = hist_prev is not None
    hp = hist_prev.astype(np.float64) if have else np.zeros((H, W, 8))
    for t in range(4):
        tx, ty = x0.astype(np.int64) + (t & 1), y0.astype(np.int64) + (t >> 1)
        w = (fx if t & 1 else 1 - fx) * (fy if t >> 1 else 1 - fy)
        inside = inr & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        txc, tyc = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
        h, gq = hp[tyc, txc], g_prev[tyc, txc]
        ok = inside & np.isfinite(h[..., :3]).all(-1) & ((gq[..., 3] > 0) == cov)
        dz = np.abs(gq[..., 7] - dist)
        tol = tau_z * dist + grad
        dn = (nrm * gq[..., 4:7]).sum(-1)
        ok_geo = ~cov | ((dz <= tol) & (dn >= cos_n))
        weighty = ok & (w > 1e-6) & cov
        margin &= ~weighty | ((np.abs(dz - tol) > 1e-4 * np.maximum(tol, 1e-6)) & (np.abs(dn - cos_n) > 1e-4))
        ok &= ok_geo
        wv = np.where(ok, w, 0.0)
        hv = np.where(ok[..., None], h, 0.0)
        sw += wv; sc += wv[..., None] * hv[..., :3]; sn += wv * hv[..., 3]; s1 += wv * hv[..., 4]; s2 += wv * hv[..., 5]
        big = ok & (w > 1e-6)
        cmax = np.maximum(cmax, np.where(big, np.abs(hv[..., :3]).max(-1), 0))
        m1max = np.maximum(m1max, np.where(big, np.abs(hv[..., 4]), 0))
        m2max = np.maximum(m2max, np.where(big, np.abs(hv[..., 5]), 0))
    hist = have & fin & inr & (sw >= 0.01)
    margin &= np.abs(sw - 0.01) > 1e-4
    inv = np.where(hist, 1.0 / np.where(sw > 0, sw, 1.0), 0.0)
    ch, nh, m1h, m2h = sc * inv[..., None], sn * inv, s1 * inv, s2 * inv
    n = np.where(hist, np.minimum(nh + 1, history_cap), 1.0)
    ac, am = np.maximum(alpha_color, 1 / n), np.maximum(alpha_moments, 1 / n)
    ci = np.where(hist[..., None], ch + ac[..., None] * (c - ch), c)
    m1 = np.where(hist, m1h + am * (L - m1h), L)
    m2 = np.where(hist, m2h + am * (L * L - m2h), L * L)
    margin_other = margin.copy()
    near4 = np.abs(n - 4) <= 1e-3
    margin &= ~near4
    v = np.where(n >= 4, np.maximum(m2 - m1 * m1, 0.0), v_frame)
    np.seterr(**old)
    return dict(ci=ci, n=n, m1=m1, m2=m2, v=v, hist=hist, margin=margin, cscale=cmax, m1scale=m1max, m2scale=m2max,
                margin_other=margin_other, near4=near4, sw=sw)


def _mirror_history(ref, fb):
    H, W = fb.shape[:2]
    fin = np.isfinite(fb[..., :3]).all(-1)
    h = np.concatenate([ref["ci"], ref["n"][..., None], ref["m1"][..., None], ref["m2"][..., None], ref["v"][..., None], np.zeros((H, W, 1))],
                       -1).astype(f32)
    h[..., :3] = np.where(fin[..., None], h[..., :3], fb[..., :3])
    return h


# ---- float64 ray casters (prt_render_guides with K = 1 and a pinhole; the motion plane) ----------------------------------------------------------

MAT_COND, MAT_DIEL, MAT_ROUGH_COND, MAT_ROUGH_DIEL = 1 << 2, 1 << 3, 1 << 10, 1 << 11
EPS, T_MAX = 1e-5, 20.0                     # pt_device.h PT_EPS, PT_INF (the farthest hit a ray has)


def _f(ptr, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(n,)).astype(np.float64)


class Caster:
    def __init__(self, scene, cfg):
        d = scene.desc
        cnt = list(d.object_count)
        meshes = C.cast(d.meshes, C.POINTER(_pkg()._capi.Mesh))
        self.mats = []                     # [1 + mesh] like the device table; [-1] the OBJ material
        self.spheres, self.quads = [], []
        for i in range(cnt[7]):
            m = meshes[i]
            self.mats.append((np.array(m.mat.color[:3], dtype=np.float64), int(m.mat.t), float(m.mat.eta[0])))
            if i < cnt[0]:
                self.spheres.append((np.array(m.pos[:3], dtype=np.float64), float(m.joker[0]), i))
            elif i >= cnt[0] + cnt[1]:
                j = np.array(m.joker[:12], dtype=np.float64)
                self.quads.append((j[0:3], j[3:6], j[6:9], j[9:12], i))
        om = C.cast(d.obj_material, C.POINTER(_pkg()._capi.Material))[0] if d.obj_material else None
        self.obj_mat = (np.array(om.color[:3], dtype=np.float64), int(om.t), float(om.eta[0])) if om else (np.zeros(3), 0, 1.0)
        T = d.triangle_count
        self.T = T
        if T:
            v = _f(d.vertices, T * 12).reshape(T, 3, 4)[..., :3]
            self.nv = _f(d.normals, T * 12).reshape(T, 3, 4)[..., :3]
            self.p0, self.e1, self.e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
            self.lo, self.hi = v.min(1), v.max(1)
        self.ntrans = cfg.active_mats & (MAT_DIEL | MAT_ROUGH_DIEL)

    def mat(self, mid):
        return self.obj_mat if mid < 0 else self.mats[mid]

    def trace(self, o, d):
        """closest hit of each ray: t (inf = none), normal as finish_closest leaves it, mesh id (-1 = OBJ)"""
        R = o.shape[0]
        best = np.full(R, T_MAX)
        nrm = np.zeros((R, 3))
        mid = np.full(R, -2)
        if self.T:
            for r in range(R):
                inv = 1.0 / np.where(d[r] == 0, 1e-300, d[r])
                t0, t1 = (self.lo - o[r]) * inv, (self.hi - o[r]) * inv
                tn, tf = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
                cand = np.nonzero((tf >= tn) & (tf > 0) & (tn < best[r]))[0]
                if cand.size == 0:
                    continue
                e1, e2, p0 = self.e1[cand], self.e2[cand], self.p0[cand]
                pv = np.cross(d[r], e2)
                det = (e1 * pv).sum(1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    inv_det = 1.0 / det
                    tv = o[r] - p0
                    u = (tv * pv).sum(1) * inv_det
                    qv = np.cross(tv, e1)
                    v = (d[r] * qv).sum(1) * inv_det
                    t = (e2 * qv).sum(1) * inv_det
                ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > EPS) & (t < best[r])
                if ok.any():
                    k = np.nonzero(ok)[0][np.argmin(t[ok])]
                    best[r] = t[k]
                    nn = self.nv[cand[k]]
                    nrm[r] = _nrm(nn[0] * (1 - u[k] - v[k]) + nn[1] * u[k] + nn[2] * v[k])
                    mid[r] = -1
        for c, rad, i in self.spheres:
            p = o - c
            B = (p * d).sum(1)
            Cc = (p * p).sum(1) - rad * rad
            det = B * B - Cc
            ok = det >= 0
            sq = np.sqrt(np.where(ok, det, 0))
            t1, t2 = -B - sq, -B + sq
            t = np.where((t1 > EPS) & (t1 < best), t1, np.where((t2 > EPS) & (t2 < best), t2, np.inf))
            hit = ok & np.isfinite(t)
            best = np.where(hit, t, best)
            nrm = np.where(hit[:, None], _nrm(o + d * t[:, None] - c), nrm)
            mid = np.where(hit, i, mid)
        for base, e0, e1, qn, i in self.quads:
            anchor = base - (e0 + e1) * 0.5
            nd = d @ qn
            with np.errstate(divide="ignore", invalid="ignore"):
                t = ((anchor - o) @ qn) / nd
            q = o + d * t[:, None]
            x0, x1 = ((q - anchor) @ e0) / (e0 @ e0), ((q - anchor) @ e1) / (e1 @ e1)
            hit = (nd > 1e-5) & (t > EPS) & (t < best) & (x0 >= 0) & (x0 <= 1) & (x1 >= 0) & (x1 <= 1)
            best = np.where(hit, t, best)
            nrm = np.where(hit[:, None], qn, nrm)
            mid = np.where(hit, i, mid)
        found = mid > -2
        best = np.where(found, best, np.inf)
        for r in np.nonzero(found)[0]:                            # finish_closest: the normal of a non-transmissive hit faces the ray
            col, t_bits, _ = self.mat(mid[r])
            if (t_bits & 0xffff & ~self.ntrans) and (nrm[r] @ d[r]) > 0:
                nrm[r] = -nrm[r]
        return best, nrm, mid

    def guides(self, cam, W, H):
        pos, view, up = (np.array(x[:3], dtype=np.float64) for x in (cam.position, cam.view, cam.up))
        view, up = _nrm(view), _nrm(up)
        h_ax = _nrm(np.cross(view, up)); v_ax = _nrm(np.cross(h_ax, view))
        horiz = h_ax * np.tan(np.radians(cam.fov[0] * 0.5)); vert = v_ax * np.tan(np.radians(cam.fov[1] * -0.5))
        ys, xs = np.mgrid[0:H, 0:W]
        sx, sy = xs / (W - 1.0), (H - ys - 1) / (H - 1.0)
        on = pos + view + horiz * (2 * sx - 1)[..., None] + vert * (2 * sy - 1)[..., None]
        img = pos + (on - pos) * cam.focalDistance
        d = _nrm(img - pos).reshape(-1, 3)
        o = np.broadcast_to(pos, d.shape).copy()
        R = d.shape[0]
        tint, dist = np.ones((R, 3)), np.zeros(R)
        out = np.zeros((R, 8))
        live = np.arange(R)
        for events in range(5):
            t, n, mid = self.trace(o[live], d[live])
            miss = ~np.isfinite(t)
            out[live[miss], 0:3] = 0.0                             # black environment
            hit_rows = np.nonzero(~miss)[0]
            nxt = []
            for j in hit_rows:
                r = live[j]
                col, tb, eta = self.mat(mid[j])
                dist[r] += t[j]
                cond = (tb & MAT_COND) and not (tb & MAT_ROUGH_COND)
                diel = (tb & MAT_DIEL) and not (tb & MAT_ROUGH_DIEL)
                if not (cond or diel) or events == 4:
                    nn = -n[j] if n[j] @ d[r] > 0 else n[j]
                    out[r] = np.concatenate([tint[r] * np.clip(col, 0, 1), [1.0], nn, [dist[r]]])
                    continue
                dd = d[r]
                c = -(n[j] @ dd)
                nd = dd - 2 * (dd @ n[j]) * n[j]
                if cond:
                    tint[r] *= np.clip(col, 0, 1)
                else:
                    e = eta if c < 0 else 1 / eta
                    ci = abs(c)
                    s2 = e * e * (1 - ci * ci)
                    if s2 <= 1:
                        nd = (dd + n[j] * c) * e - n[j] * np.copysign(np.sqrt(1 - s2), c)
                o[r] = o[r] + dd * t[j]
                d[r] = _nrm(nd)
                nxt.append(r)
            live = np.array(nxt, dtype=np.int64)
            if live.size == 0:
                break
        return out.reshape(H, W, 8)


# the largest |D - caster's D| over the matching pixels measured on an MI355X (cornell_coat, seed 11; DESIGN.md s4 "Motion"), and the bound: 4 x
# that -- never looser than 1e-3 of the mesh's bounding-box diagonal, under which a wrong vertex or swapped (u, v) (an edge length off) cannot fit
D_MEASURED = 1.1e-7
D_BOUND = 4 * D_MEASURED


class MotionCaster(Caster):
    """Caster on given vertices; first_hits() also names the triangle and barycentrics of every primary ray that ends on the mesh"""

    def __init__(self, scene, cfg, vertices):
        super().__init__(scene, cfg)
        v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3, 4)[..., :3]
        self.vtx = v
        self.p0, self.e1, self.e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        self.lo, self.hi = v.min(1), v.max(1)

    def first_hits(self, cam, W, H):
        """per pixel of the pinhole centre rays: mesh (the first hit is a mesh triangle of a non-delta material), tri, u, v"""
        B = camera_basis(cam)
        d = centre_dirs(B, W, H).reshape(-1, 3)
        o = np.broadcast_to(B[0], d.shape).copy()
        t, n, mid = self.trace(o, d)
        col, tb, eta = self.obj_mat
        delta = bool(((tb & MAT_COND) and not (tb & MAT_ROUGH_COND)) or ((tb & MAT_DIEL) and not (tb & MAT_ROUGH_DIEL)))
        R = d.shape[0]
        mesh = np.isfinite(t) & (mid == -1) & (not delta)
        tri, uu, vv = np.zeros(R, dtype=np.int64), np.zeros(R), np.zeros(R)
        for r in np.nonzero(mesh)[0]:
            pv = np.cross(d[r], self.e2)
            det = (self.e1 * pv).sum(1)
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / det
                tv = o[r] - self.p0
                u = (tv * pv).sum(1) * inv
                qv = np.cross(tv, self.e1)
                v = (d[r] * qv).sum(1) * inv
                tt = (self.e2 * qv).sum(1) * inv
            ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (tt > EPS)
            k = np.nonzero(ok)[0][np.argmin(tt[ok])]
            assert abs(tt[k] - t[r]) <= 1e-9 * max(t[r], 1.0)
            tri[r], uu[r], vv[r] = k, u[k], v[k]
        # pixels whose first hit is a smooth conductor (a mirror) and whose reflected ray ends on the mesh: the mesh behind a delta chain
        mirror = np.zeros(R, dtype=bool)
        for r in np.nonzero(np.isfinite(t) & (mid >= 0))[0]:
            tb_r = self.mat(mid[r])[1]
            mirror[r] = bool((tb_r & MAT_COND) and not (tb_r & MAT_ROUGH_COND))
        behind = np.zeros(R, dtype=bool)
        rows = np.nonzero(mirror)[0]
        if rows.size:
            o2 = o[rows] + d[rows] * t[rows, None]
            d2 = d[rows] - 2 * (d[rows] * n[rows]).sum(-1, keepdims=True) * n[rows]
            d2 = d2 / np.linalg.norm(d2, axis=-1, keepdims=True)
            t2, _, mid2 = self.trace(o2, d2)
            behind[rows] = np.isfinite(t2) & (mid2 == -1)
        shp = (H, W)
        return (mesh.reshape(shp), tri.reshape(shp), uu.reshape(shp), vv.reshape(shp), mid.reshape(shp), np.isfinite(t).reshape(shp),
                np.where(np.isfinite(t), t, 0.0).reshape(shp), behind.reshape(shp))


def _point(vtx, tri, u, v):
    a = vtx[tri]
    return a[..., 0, :] * (1 - u - v)[..., None] + a[..., 1, :] * u[..., None] + a[..., 2, :] * v[..., None]


# ---- known answers: the reference's functions, the OpenCL sampler rules --------------------------------------------------------------------------

def kat_tables():
    g = np.load(os.path.join(GOLDEN, "kat_functions.npz"))
    for name in sorted({k.split("/")[0] for k in g.files}):
        yield name, int(g[name + "/fn"]), g[name + "/params"], g[name + "/cases"], g[name + "/expect"], g[name + "/cols"]


def assert_kat_equal(name, got, expect, cols):
    a = np.ascontiguousarray(got[:, cols]).view(np.uint32).copy()
    b = np.ascontiguousarray(expect[:, cols]).view(np.uint32).copy()
    both_nan = np.isnan(got[:, cols]) & np.isnan(expect[:, cols])
    a[both_nan] = 0
    b[both_nan] = 0
    bad = np.argwhere(a != b)
    assert bad.size == 0, "%s: %d of %d cases differ, first: case %d column %d got %r expected %r" % (
        name, len(set(bad[:, 0].tolist())), got.shape[0], bad[0, 0], cols[bad[0, 1]], got[bad[0, 0], cols[bad[0, 1]]], expect[bad[0, 0], cols[bad[0, 1]]])


def _env_cases():
    """environment lookups with answers worked out from the OpenCL 1.2 specification (s8.2, CLK_FILTER_LINEAR with
    normalized coordinates, CLK_ADDRESS_CLAMP = transparent black border, kernels/main.cl:25) in float64: the direction
    maps to (s, t) = (atan2(z, x) / 2pi + 1/2, acos(y) / pi) (kernels/utils.cl:46); u = s w, i0 = floor(u - 1/2),
    a = frac(u - 1/2), likewise v, j0, b; result = (1-a)(1-b) T[i0,j0] + a(1-b) T[i0+1,j0] + (1-a)b T[i0,j0+1] + ab T[i0+1,j0+1]
    with T = 0 outside the image.  Independent of the product's code and of the shim the reference build links."""
    import math
    rng = np.random.default_rng(7)
    tables = []
    for w, h in ((1, 1), (2, 1), (4, 2), (5, 3)):
        tex = rng.uniform(0.1, 4.0, (h, w, 3))
        dirs = []
        for j in range(h):                                     # texel centres: the texel itself, exactly
            for i in range(w):
                s, t = (i + 0.5) / w, (j + 0.5) / h
                phi, theta = (s - 0.5) * 2 * math.pi, t * math.pi
                dirs.append((math.sin(theta) * math.cos(phi), math.cos(theta), math.sin(theta) * math.sin(phi)))
        dirs += [(0, 1, 0), (0, -1, 0), (-1, 0, 0), (-1, 0, 1e-6), (-1, 0, -1e-6), (1, 0, 0)]     # poles, the seam (s = 0 / 1: half border), s = 1/2
        v = rng.normal(size=(40, 3))
        dirs += (v / np.linalg.norm(v, axis=1, keepdims=True)).tolist()
        dirs = np.array(dirs, dtype=np.float32)
        expect = np.zeros((len(dirs), 3))
        for n, d in enumerate(dirs.astype(np.float64)):
            s = math.atan2(d[2], d[0]) / (2 * math.pi) + 0.5
            t = math.acos(max(-1.0, min(1.0, d[1]))) / math.pi
            u, vv = s * w, t * h
            i0, j0 = math.floor(u - 0.5), math.floor(vv - 0.5)
            a, b = (u - 0.5) - i0, (vv - 0.5) - j0
            def T(i, j):
                return tex[j, i] if 0 <= i < w and 0 <= j < h else np.zeros(3)
            expect[n] = (1 - a) * (1 - b) * T(i0, j0) + a * (1 - b) * T(i0 + 1, j0) + (1 - a) * b * T(i0, j0 + 1) + a * b * T(i0 + 1, j0 + 1)
        params = np.zeros(80, dtype=np.float32)
        params[0:2] = np.array([w, h], dtype=np.uint32).view(np.float32)
        params[2:2 + 3 * w * h] = tex.astype(np.float32).reshape(-1)
        cases = np.zeros((len(dirs), 32), dtype=np.float32)
        cases[:, 0:3] = dirs
        tables.append(("%dx%d" % (w, h), params, cases, expect, tex.astype(np.float32)))
    return tables


def check_env_lookup(run):
    for name, params, cases, expect, tex in _env_cases():
        got = run(11, params, cases)[:, 0:3].astype(np.float64)
        # float32 atan2 / acos (<= 3 ulp) move the sample point by ~1e-6 texel: values agree to ~1e-5 of the texel range
        err = np.abs(got - expect).max(-1)
        assert np.allclose(got, expect, rtol=0, atol=4e-5 * float(tex.max())), "%s: the lookup of direction %d is %.3g from the specification's answer (allowed %.3g)" % (
            name, int(np.argmax(err)), err.max(), 4e-5 * float(tex.max()))
        n_tex = tex.shape[0] * tex.shape[1]
        centre = got[:n_tex].reshape(tex.shape)
        assert np.allclose(centre, tex, rtol=2e-6, atol=0), name + ": a lookup at a texel centre must return that texel"
