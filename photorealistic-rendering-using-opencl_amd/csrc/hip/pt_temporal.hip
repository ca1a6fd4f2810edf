// pt_temporal.hip -- temporal reprojection in front of the a-trous filter (prt_denoise_temporal; include/prt.h has the contract).
// A translation unit of its own: no code object of the render kernels or of pt_denoise.hip changes with it.
//
//   tm_reproject_kernel  per pixel: the world point of the current guides, projected into the previous camera; the valid ones of the 2x2
//                        bilinear taps of the previous history and guides blended with the framebuffer into {c_i, v} (the filter's input)
//                        and the new history {c, n}, {m1, m2, v, 0}
//   tm_feedback_kernel   PRT_TEMPORAL_FEEDBACK_ATROUS: a-trous pass 0's colour into the new history
// With a temporal response (prt.h prt_set_temporal_response) the reprojection is the kernel's <true> instance, which also blends the
// fast history f_i from the same taps, and a pass of its own follows it:
//   tm_clamp_kernel      per pixel: mean and deviation of f_i over the (2 radius + 1)^2 window, from a tile of f_i staged in LDS; c_i clamped
//                        to mean +- k sigma, into the filter's input and the new history; a clamped pixel's n is cut to fast_cap
//
// The history is double-buffered (taps read neighbours: never updated in place); the caller flips the two halves after each call.  16x16
// workgroups, one lane per pixel, straight global loads as the filter's kernels: at 1080p the planes a call touches (~100 B per pixel) stay
// in the L2 / Infinity Cache.  A pixel reads its 2x2 taps (2 guide float4 + 2 history float4 each) and its own and four neighbours' guides.
#include "pt_denoise_dev.h"
#include "pt_launch.h"

namespace prt {
using namespace dev;

struct TmParams { float alpha_color, alpha_moments, tau_z, cos_n, cap; int has_hist; };

// fb: framebuffer; var: dn_var_kernel's {c, v} of the current frame (v for n < 4); gd / gd_prev: current / previous guides (2 float4 per
// pixel); h_cn_prev / h_m_prev: previous history {c, n} / {m1, m2, v, 0}.  Out: {c_i, v} and the new history.
// motion: null, or the motion plane {D, m} of the current guides (prt.h prt_set_motion): a covered pixel with m > 0 and D != 0 reprojects
// X + D, where its surface point was, instead of X; every other pixel -- and so a plane of zeros -- takes today's expressions
// RESP (prt.h prt_set_temporal_response): f_prev / f_out the fast history {f.rgb, took the history branch} of the previous call / of this
// one, fast_cap its length; the had-history word also goes into the spare lane of h_m, where tm_clamp_kernel leaves the pixel's flag.
// Without RESP none of the three is read: the <false> instance has the instructions the kernel had before it became a template
template <bool RESP>
__global__ __launch_bounds__(256) void tm_reproject_kernel(const float4* __restrict__ fb, const float4* __restrict__ var,
                                                           const float4* __restrict__ gd, const float4* __restrict__ gd_prev,
                                                           const float4* __restrict__ h_cn_prev, const float4* __restrict__ h_m_prev,
                                                           const DevCamera cur, const DevCamera prev, int W, int H, const TmParams P,
                                                           float4* __restrict__ out, float4* __restrict__ h_cn, float4* __restrict__ h_m,
                                                           const float4* __restrict__ motion, const float4* __restrict__ f_prev,
                                                           float4* __restrict__ f_out, float fast_cap) {
    const int x = (int)(blockIdx.x * 16 + threadIdx.x), y = (int)(blockIdx.y * 16 + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t id = (size_t)y * W + x;
    const float4 c = fb[id];
    const float L = dn_lum(c.x, c.y, c.z);
    float sw = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hn = 0.0f, h1 = 0.0f, h2 = 0.0f;
    float fr = 0.0f, fg = 0.0f, fbl = 0.0f;
    if (P.has_hist && dn_finite3(c)) {
        const float4 ap = gd[2 * id], np = gd[2 * id + 1];
        const bool covp = ap.w > 0.0f;
        // create_cam_ray's centre ray of the pixel (pt_device.h), then the point at its guide depth
        const float sx = (float)x / (W - 1.0f);
        const float sy = (float)(H - y - 1) / (H - 1.0f);
        const f3 position = ld3(cur.position);
        const f3 onPlane = ld3(cur.middle) + (ld3(cur.horizontal) * ((2 * sx) - 1)) + (ld3(cur.vertical) * ((2 * sy) - 1));
        const f3 d = normalize(onPlane - position);
        const f3 Pp = ld3(prev.position), Hz = ld3(prev.horizontal), Vt = ld3(prev.vertical);
        const f3 f = ld3(prev.middle) - Pp;
        f3 X = position + d * np.w;
        if (motion && covp) {
            const float4 mv = motion[id];
            if (mv.w > 0.0f && (mv.x != 0.0f || mv.y != 0.0f || mv.z != 0.0f)) X = X + F3(mv.x, mv.y, mv.z);
        }
        const f3 e = covp ? X - Pp : d;
        const float dist = covp ? length(e) : 0.0f;
        const float ef = dot(e, f);
        if (ef > 0.0f) {
            const f3 q = e * (dot(f, f) / ef) - f;
            const float a = dot(q, Hz) / dot(Hz, Hz), b = dot(q, Vt) / dot(Vt, Vt);
            const float xp = (a + 1.0f) * 0.5f * (float)(W - 1);
            const float yp = (float)(H - 1) - (b + 1.0f) * 0.5f * (float)(H - 1);
            if (xp > -1.0f && xp < (float)W && yp > -1.0f && yp < (float)H) {
                const float x0f = floorf(xp), y0f = floorf(yp);
                const int x0 = (int)x0f, y0 = (int)y0f;
                const float fx = xp - x0f, fy = yp - y0f;
                const float grad = covp ? fmaxf(dn_grad1(gd, x, y, 1, 0, W, H, np.w), dn_grad1(gd, x, y, 0, 1, W, H, np.w)) : 0.0f;
                const float ztol = P.tau_z * dist + grad;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
                    if (tx < 0 || tx >= W || ty < 0 || ty >= H) continue;
                    const size_t qi = (size_t)ty * W + tx;
                    const float4 hc = h_cn_prev[qi];
                    if (!dn_finite3(hc)) continue;
                    if ((gd_prev[2 * qi].w > 0.0f) != covp) continue;
                    if (covp) {
                        const float4 nq = gd_prev[2 * qi + 1];
                        if (!(fabsf(nq.w - dist) <= ztol)) continue;
                        if (!(np.x * nq.x + np.y * nq.y + np.z * nq.z >= P.cos_n)) continue;
                    }
                    const float w = ((t & 1) ? fx : 1.0f - fx) * ((t >> 1) ? fy : 1.0f - fy);
                    const float4 hm = h_m_prev[qi];
                    sw += w;
                    hr += w * hc.x; hg += w * hc.y; hb += w * hc.z; hn += w * hc.w;
                    h1 += w * hm.x; h2 += w * hm.y;
                    if (RESP) {
                        const float4 fq = f_prev[qi];
                        fr += w * fq.x; fg += w * fq.y; fbl += w * fq.z;
                    }
                }
            }
        }
    }
    float4 ci;
    float n, m1, m2;
    if (sw >= 0.01f) {
        const float inv = 1.0f / sw;
        const float chr = hr * inv, chg = hg * inv, chb = hb * inv, m1h = h1 * inv, m2h = h2 * inv;
        n = fminf(hn * inv + 1.0f, P.cap);
        const float ac = fmaxf(P.alpha_color, 1.0f / n), am = fmaxf(P.alpha_moments, 1.0f / n);
        ci = make_float4(chr + ac * (c.x - chr), chg + ac * (c.y - chg), chb + ac * (c.z - chb), c.w);
        m1 = m1h + am * (L - m1h);
        m2 = m2h + am * (L * L - m2h);
        if (RESP) {
            const float fhr = fr * inv, fhg = fg * inv, fhb = fbl * inv;
            const float af = 1.0f / fminf(hn * inv + 1.0f, fast_cap);
            f_out[id] = make_float4(fhr + (c.x - fhr) * af, fhg + (c.y - fhg) * af, fhb + (c.z - fhb) * af, 1.0f);
        }
    } else {
        n = 1.0f;
        ci = c;
        m1 = L;
        m2 = L * L;
        if (RESP) f_out[id] = make_float4(c.x, c.y, c.z, 0.0f);
    }
    const float v = n >= 4.0f ? fmaxf(m2 - m1 * m1, 0.0f) : var[id].w;
    out[id] = make_float4(ci.x, ci.y, ci.z, v);
    h_cn[id] = make_float4(ci.x, ci.y, ci.z, n);
    h_m[id] = make_float4(m1, m2, v, RESP && sw >= 0.01f ? 1.0f : 0.0f);
}

// the clamp of prt.h prt_set_temporal_response, window radius R.  fast: this call's fast history {f_i.rgb, took the history branch}, read
// with its neighbours; io (the filter's input {c_i, v}), h_cn ({c_i, n}) and the spare lane of h_m (the flag) are read and written at the
// lane's own pixel only.  The block's 16x16 pixels and a halo of R are staged once as float4 texels {f.rgb, valid}: a texel outside the frame
// or with a non-finite channel is marked invalid, never clamped into the frame.  Every lane of the block stages and reaches the barrier;
// lanes outside the frame leave behind it
template <int R>
__global__ __launch_bounds__(256) void tm_clamp_kernel(const float4* __restrict__ fast, int W, int H, float k, float fast_cap,
                                                       float4* __restrict__ io, float4* __restrict__ h_cn, float4* __restrict__ h_m) {
    constexpr int T = 16 + 2 * R;
    __shared__ float4 tile[T * T];
    const int bx = (int)(blockIdx.x * 16) - R, by = (int)(blockIdx.y * 16) - R;
    for (int i = (int)(threadIdx.y * 16 + threadIdx.x); i < T * T; i += 256) {
        const int gx = bx + i % T, gy = by + i / T;
        float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const float4 g = fast[(size_t)gy * W + gx];
            if (dn_finite3(g)) f = make_float4(g.x, g.y, g.z, 1.0f);
        }
        tile[i] = f;                                                   // an invalid texel is all zeros
    }
    __syncthreads();
    const int x = (int)(blockIdx.x * 16 + threadIdx.x), y = (int)(blockIdx.y * 16 + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t id = (size_t)y * W + x;
    if (!(fast[id].w > 0.0f)) return;                                  // no history: the pixel passes through
    const float4 cn = h_cn[id];
    if (!dn_finite3(cn)) return;
    const float4* t0 = tile + threadIdx.y * T + threadIdx.x;           // the window's first texel: (x - R, y - R)
    float m = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
    for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
        for (int dx = 0; dx <= 2 * R; ++dx) {
            const float4 f = t0[dy * T + dx];                         // (an invalid texel adds +0 to sums that are never -0: left out exactly)
            m += f.w; sr += f.x; sg += f.y; sb += f.z;
        }
    if (!(m >= 1.0f)) return;
    const float mr = sr / m, mg = sg / m, mb = sb / m;
    float qr = 0.0f, qg = 0.0f, qb = 0.0f;
#pragma unroll
    for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
        for (int dx = 0; dx <= 2 * R; ++dx) {
            const float4 f = t0[dy * T + dx];
            if (f.w > 0.0f) {
                const float er = f.x - mr, eg = f.y - mg, eb = f.z - mb;
                qr += er * er; qg += eg * eg; qb += eb * eb;
            }
        }
    const float dr = k * sqrtf(qr / m), dg = k * sqrtf(qg / m), db = k * sqrtf(qb / m);
    const float cr = fminf(fmaxf(cn.x, mr - dr), mr + dr), cg = fminf(fmaxf(cn.y, mg - dg), mg + dg), cb = fminf(fmaxf(cn.z, mb - db), mb + db);
    if (cr != cn.x || cg != cn.y || cb != cn.z) {
        io[id] = make_float4(cr, cg, cb, io[id].w);
        h_cn[id] = make_float4(cr, cg, cb, fminf(cn.w, fast_cap));
        h_m[id].w = 2.0f;
    }
}

__global__ __launch_bounds__(256) void tm_feedback_kernel(const float4* __restrict__ pass0, int W, int H, float4* __restrict__ h_cn) {
    const int x = (int)(blockIdx.x * 16 + threadIdx.x), y = (int)(blockIdx.y * 16 + threadIdx.y);
    if (x >= W || y >= H) return;
    const size_t id = (size_t)y * W + x;
    const float4 p = pass0[id];
    h_cn[id] = make_float4(p.x, p.y, p.z, h_cn[id].w);
}

// the temporal steps of launch_filter_chain (pt_denoise.hip), which says where `var` and `in` are
void launch_temporal_front(const FilterPlanes& pl, const float4* var, float4* in, const prt_temporal_params& t, const DevCamera& cam,
                           const TemporalHistory& h, const float4* motion, hipStream_t stream) {
    const dim3 blk = dn_block(), grd = dn_grid(pl.W, pl.H);
    const int W = pl.W, H = pl.H;
    TmParams P;
    P.alpha_color = t.alpha_color; P.alpha_moments = t.alpha_moments; P.tau_z = t.tau_z; P.cos_n = t.cos_n; P.cap = (float)t.history_cap;
    P.has_hist = h.valid ? 1 : 0;
    if (!h.fast) {
        hipLaunchKernelGGL(tm_reproject_kernel<false>, grd, blk, 0, stream, pl.fb, var, pl.guides, h.guides_prev, h.cn_prev, h.m_prev, cam,
                           h.cam_prev, W, H, P, in, h.cn, h.m, motion, nullptr, nullptr, 0.0f);
    } else {
        const float fast_cap = (float)h.fast_cap;
        hipLaunchKernelGGL(tm_reproject_kernel<true>, grd, blk, 0, stream, pl.fb, var, pl.guides, h.guides_prev, h.cn_prev, h.m_prev, cam,
                           h.cam_prev, W, H, P, in, h.cn, h.m, motion, h.fast_prev, h.fast, fast_cap);
        if (h.radius == 1) hipLaunchKernelGGL(tm_clamp_kernel<1>, grd, blk, 0, stream, h.fast, W, H, h.k, fast_cap, in, h.cn, h.m);
        else if (h.radius == 2) hipLaunchKernelGGL(tm_clamp_kernel<2>, grd, blk, 0, stream, h.fast, W, H, h.k, fast_cap, in, h.cn, h.m);
        else hipLaunchKernelGGL(tm_clamp_kernel<3>, grd, blk, 0, stream, h.fast, W, H, h.k, fast_cap, in, h.cn, h.m);
    }
}
void launch_temporal_feedback(const float4* pass0, int W, int H, float4* h_cn, hipStream_t stream) {
    hipLaunchKernelGGL(tm_feedback_kernel, dn_grid(W, H), dn_block(), 0, stream, pass0, W, H, h_cn);
}

}  // namespace prt
