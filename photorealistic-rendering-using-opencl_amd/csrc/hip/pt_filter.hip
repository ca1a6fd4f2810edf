// pt_filter.hip -- host side of the pixel filter (prt_set_pixel_filter, include/prt.h): the inverse-CDF table of the Gaussian and
// Blackman-Harris kinds, and the device self-test of pt_filter.h (prt_selftest_fn fn 12).  The render kernels' filter builds are the
// pt_inst_filter_*.hip files.
#include <cmath>

#include "pt_filter.h"
#include "pt_launch.h"

namespace prt {
using namespace dev;

// prt.h: T[i] = F^-1(i / 256) in float64, rounded to f32, F the normalised CDF of the kind's profile on [-r, r] in closed form.  Computed for
// r = 1 (the profiles scale with r: sigma = r / 3, cos(pi x / r)) and multiplied by r; built antisymmetric, T[128] = 0
static double filter_cdf1(unsigned kind, double x) {
    const double pi = 3.14159265358979323846;
    if (kind == PRT_FILTER_GAUSSIAN) {
        const double s = 1.0 / 3.0, c = std::exp(-1.0 / (2.0 * s * s));
        auto G = [&](double t) { return s * std::sqrt(pi / 2.0) * std::erf(t / (s * std::sqrt(2.0))) - c * t; };
        return (G(x) - G(-1.0)) / (G(1.0) - G(-1.0));
    }
    const double a0 = 0.35875, a1 = 0.48829, a2 = 0.14128, a3 = 0.01168;     // Blackman-Harris
    auto G = [&](double t) { return a0 * t + a1 / pi * std::sin(pi * t) + a2 / (2.0 * pi) * std::sin(2.0 * pi * t) + a3 / (3.0 * pi) * std::sin(3.0 * pi * t); };
    return (G(x) - G(-1.0)) / (G(1.0) - G(-1.0));
}

void build_filter_table(unsigned kind, float r, float* tab) {
    tab[0] = -r; tab[PT_FILTER_TAB] = r; tab[PT_FILTER_TAB / 2] = 0.0f;
    for (int i = 1; i < PT_FILTER_TAB / 2; ++i) {
        const double p = (double)i / PT_FILTER_TAB;
        double lo = -1.0, hi = 0.0;                                  // F is increasing, F(0) = 1/2 > p
        for (int it = 0; it < 200 && hi - lo > 1e-17; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (filter_cdf1(kind, mid) < p) lo = mid; else hi = mid;
        }
        tab[i] = (float)((double)r * (0.5 * (lo + hi)));
        tab[PT_FILTER_TAB - i] = -tab[i];
    }
}

__global__ void selftest_filter_kernel(unsigned kind, float r, const float* __restrict__ tab, const float* __restrict__ in, float* __restrict__ out, int n) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const float* x = in + 32 * (size_t)i;
    float* y = out + 32 * (size_t)i;
    float dx, dy;
    filter_offset(kind, r, tab, __float_as_uint(x[0]), __float_as_uint(x[1]), __float_as_uint(x[2]), dx, dy);
    for (int k = 2; k < 32; ++k) y[k] = 0.0f;
    y[0] = dx; y[1] = dy;
}

void launch_selftest_filter(unsigned kind, float r, const float* tab, const float* in, float* out, int n, hipStream_t stream) {
    hipLaunchKernelGGL(selftest_filter_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, kind, r, tab, in, out, n);
}

}  // namespace prt
