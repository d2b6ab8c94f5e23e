// The reference's warp test (src/utils/warptest.cpp, runTest and what it calls) on the device, over the warp, BSDF and
// phase device functions the render kernels call.
//
//   warp_histogram_kernel   generatePoints (Independent) and the binning loop (warptest.cpp:146-168, :457-479). Built as
//                           chi2_histogram_kernel is: a lane owns a contiguous run of points -- one pcg_advance to its
//                           first draw, then three sequential draws of the default-state pcg32 per point -- and counts
//                           into a uint32 table in LDS with integer atomics, one table per wave where four fit; a
//                           workgroup's non-zero cells then go into the global table, integer atomics again. Points
//                           with a NaN coordinate are tallied the same way, beside the table. The warp type is uniform
//                           over the launch: the kernel switches on it once, outside the point loop.
//   warp_expected_kernel    the expected frequencies (warptest.cpp:481-551): one lane per cell runs adaptiveSimpson2D
//                           (nh_simpson.h) of the type's pdf. Throughput is not this kernel's business.
//   warp_query_kernel       warpPoint (warptest.cpp:102-131) or the matching pdf, one lane per query.
//
// Built once, with -DNH_DISNEY (Makefile), as nh_chi2.hip is.
#include "nh_internal.h"
#include "nh_simpson.h"
#include "nh_volume.h"

#ifndef NH_DISNEY
#error "nh_warp.hip is built with -DNH_DISNEY"
#endif

using namespace nhd;

namespace nh_disney {

namespace {
constexpr float kWarpInvTwoPi = 0.15915494309189533577f;  // INV_TWOPI (common.h)

__device__ __forceinline__ int warp_clamp_bin(int v, int res) { return min(max(0, v), res - 1); }

__device__ __forceinline__ Medium warp_phase(int type, float g) {
    Medium m;
    m.homog = false;
    m.mu_t = f3(0, 0, 0);
    m.phase = type == NH_WARP_ISO_PHASE ? PHASE_ISO : PHASE_HG;
    m.g = g;
    return m;
}

// warpPoint (warptest.cpp:102-131): the warped point and its weight
template <int TYPE>
__device__ __forceinline__ float warp_point(const WarpSpec &w, float sx, float sy, float sz, F3 &p) {
    if constexpr (TYPE == NH_WARP_NONE) {
        p = f3(sx, sy, 0.f);  // squareToUniformSquare (warp.cpp:41)
    } else if constexpr (TYPE == NH_WARP_DISK) {
        uniform_disk(sx, sy, p.x, p.y);
        p.z = 0.f;
    } else if constexpr (TYPE == NH_WARP_UNIFORM_SPHERE) {
        p = uniform_sphere(sx, sy);
    } else if constexpr (TYPE == NH_WARP_UNIFORM_SPHERE_VOL) {
        p = uniform_sphere_volume(sx, sy, sz);
    } else if constexpr (TYPE == NH_WARP_UNIFORM_SPHERE_CAP) {
        p = uniform_sphere_cap(sx, sy, w.parameter);
    } else if constexpr (TYPE == NH_WARP_UNIFORM_HEMISPHERE) {
        p = uniform_hemisphere(sx, sy);
    } else if constexpr (TYPE == NH_WARP_COSINE_HEMISPHERE) {
        p = cosine_hemisphere(sx, sy);
    } else if constexpr (TYPE == NH_WARP_BECKMANN) {
        p = beckmann(sx, sy, w.parameter);
    } else if constexpr (TYPE == NH_WARP_HENYEY_GREENSTEIN) {
        p = henyey_greenstein(sx, sy, w.parameter);
    } else if constexpr (TYPE == NH_WARP_MICROFACET_BRDF) {  // :117-121
        const F3 wi = f3(w.wi[0], w.wi[1], w.wi[2]), alb = f3(0, 0, 0);
        int measure;
        const F3 c = bsdf_sample(w.bsdf, wi, sx, sy, p, measure, alb);
        const float value = c.x * 0.212671f + c.y * 0.715160f + c.z * 0.072169f;  // Color3f::getLuminance
        return value == 0 ? 0.f : bsdf_eval(w.bsdf, wi, p, M_SOLID_ANGLE, alb).x;
    } else {  // NH_WARP_ISO_PHASE, NH_WARP_ANISO_PHASE (:122-127)
        p = phase_sample(warp_phase(TYPE, w.parameter), sx, sy);
    }
    return 1.f;
}

// the matching *Pdf of a point (warptest.cpp:481-529 names them)
__device__ __forceinline__ float warp_pdf(const WarpSpec &w, F3 v) {
    switch (w.type) {
        case NH_WARP_NONE: return uniform_square_pdf(v.x, v.y);
        case NH_WARP_DISK: return uniform_disk_pdf(v.x, v.y);
        case NH_WARP_UNIFORM_SPHERE: return uniform_sphere_pdf(v);
        case NH_WARP_UNIFORM_SPHERE_VOL: return uniform_sphere_volume_pdf();
        case NH_WARP_UNIFORM_SPHERE_CAP: return uniform_sphere_cap_pdf(v, w.parameter);
        case NH_WARP_UNIFORM_HEMISPHERE: return uniform_hemisphere_pdf(v);
        case NH_WARP_COSINE_HEMISPHERE: return cosine_hemisphere_pdf(v);
        case NH_WARP_BECKMANN: return beckmann_pdf(v, w.parameter);
        case NH_WARP_MICROFACET_BRDF: return bsdf_pdf(w.bsdf, f3(w.wi[0], w.wi[1], w.wi[2]), v, M_SOLID_ANGLE);
        case NH_WARP_HENYEY_GREENSTEIN:
        case NH_WARP_ISO_PHASE:
        case NH_WARP_ANISO_PHASE: return phase_pdf(warp_phase(w.type, w.parameter), v);
    }
    return 0.f;
}

// The cell of a point (warptest.cpp:463-478), or -1 for a point with a NaN coordinate: the reference's (int) cast of a
// NaN is undefined, so such a point is tallied and not counted
template <int TYPE>
__device__ __forceinline__ int warp_cell(F3 p, int xres, int yres) {
    float x, y;
    if constexpr (TYPE == NH_WARP_NONE) {
        x = p.x;
        y = p.y;
    } else if constexpr (TYPE == NH_WARP_DISK) {
        x = p.x * 0.5f + 0.5f;
        y = p.y * 0.5f + 0.5f;
    } else {
        x = f_atan2(p.y, p.x) * kWarpInvTwoPi;
        if (x < 0) x += 1;
        y = p.z * 0.5f + 0.5f;
    }
    if (x != x || y != y) return -1;
    const int xbin = warp_clamp_bin((int)floorf(x * (float)xres), xres);
    const int ybin = warp_clamp_bin((int)floorf(y * (float)yres), yres);
    return ybin * xres + xbin;  // xbin < xres and ybin < yres: inside the table
}

// a lane's run of points: count of them from the stream position rng is at
template <int TYPE>
__device__ __forceinline__ void warp_run(const WarpHist &h, Rng rng, int count, uint32_t *tab, uint32_t *nan_tally) {
    for (int k = 0; k < count; ++k) {
        // Point3f(nextFloat(), nextFloat(), nextFloat()): g++ evaluates the last argument first (h.rtl)
        const float a = rng.next1d(), b = rng.next1d(), c = rng.next1d();
        F3 p;
        const float weight = warp_point<TYPE>(h.w, h.rtl ? c : a, b, h.rtl ? a : c, p);
        if (weight == 0) continue;  // values(0, i) == 0
        const int cell = warp_cell<TYPE>(p, h.xres, h.yres);
        if (cell < 0) atomicAdd(nan_tally, 1u);
        else atomicAdd(&tab[cell], 1u);
    }
}
}  // namespace

__global__ __launch_bounds__(kChi2Block) void warp_histogram_kernel(WarpHist h) {
    extern __shared__ uint32_t s_warp[];  // [0]: the NaN tally; then cells entries, or kChi2Block / 64 tables of them
    uint32_t *s_tab = s_warp + 1;
    const int cells = h.xres * h.yres;
    const int n_tab = h.sub_tables ? kChi2Block / 64 : 1;
    for (int i = threadIdx.x; i < n_tab * cells + 1; i += kChi2Block) s_warp[i] = 0u;
    __syncthreads();
    uint32_t *tab = s_tab + (h.sub_tables ? (int)(threadIdx.x >> 6) * cells : 0);
    const int64_t lane = (int64_t)blockIdx.x * kChi2Block + threadIdx.x;
    const int64_t begin = lane * h.run;
    if (begin < (int64_t)h.n) {
        const int count = (int)min((int64_t)h.run, (int64_t)h.n - begin);
        Rng rng;
        rng.inc = kPcgDefaultStream;
        rng.state = pcg_advance(kPcgDefaultState, kPcgDefaultStream, h.first_draw + 3 * (uint64_t)begin);
        switch (h.w.type) {  // uniform over the launch
#define NH_WARP_CASE(T) case T: warp_run<T>(h, rng, count, tab, s_warp); break;
            NH_WARP_CASE(NH_WARP_NONE)
            NH_WARP_CASE(NH_WARP_DISK)
            NH_WARP_CASE(NH_WARP_UNIFORM_SPHERE)
            NH_WARP_CASE(NH_WARP_UNIFORM_SPHERE_VOL)
            NH_WARP_CASE(NH_WARP_UNIFORM_SPHERE_CAP)
            NH_WARP_CASE(NH_WARP_UNIFORM_HEMISPHERE)
            NH_WARP_CASE(NH_WARP_COSINE_HEMISPHERE)
            NH_WARP_CASE(NH_WARP_BECKMANN)
            NH_WARP_CASE(NH_WARP_HENYEY_GREENSTEIN)
            NH_WARP_CASE(NH_WARP_MICROFACET_BRDF)
            NH_WARP_CASE(NH_WARP_ISO_PHASE)
            NH_WARP_CASE(NH_WARP_ANISO_PHASE)
#undef NH_WARP_CASE
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += kChi2Block) {
        uint32_t v = s_tab[i];
        for (int t = 1; t < n_tab; ++t) v += s_tab[t * cells + i];
        if (v) atomicAdd(&h.counts[i], v);
    }
    if (threadIdx.x == 0 && s_warp[0]) atomicAdd(h.nan_points, s_warp[0]);
}

__global__ __launch_bounds__(64) void warp_expected_kernel(WarpExpected q) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= q.xres * q.yres) return;
    const int y = idx / q.xres, x = idx - y * q.xres;
    // warptest.cpp:540-545: (y + 1 - Epsilon) is fp32 (Epsilon is a float), the division fp64
    const double y_start = y / (double)q.yres, y_end = (double)((float)(y + 1) - kEps) / (double)q.yres;
    const double x_start = x / (double)q.xres, x_end = (double)((float)(x + 1) - kEps) / (double)q.xres;
    const WarpSpec w = q.w;
    uint32_t evals = 0;
    const auto integrand = [&](double yy, double xx) -> double {  // warptest.cpp:481-529
        ++evals;
        if (w.type == NH_WARP_NONE) return (double)uniform_square_pdf((float)xx, (float)yy);
        if (w.type == NH_WARP_DISK) {
            xx = xx * 2 - 1;
            yy = yy * 2 - 1;
            return (double)uniform_disk_pdf((float)xx, (float)yy);
        }
        xx *= (double)(2 * kPi);  // 2 * M_PI with the float M_PI
        yy = yy * 2 - 1;
        const double sin_theta = sqrt(1 - yy * yy);
        const double sin_phi = sin(xx), cos_phi = cos(xx);
        return (double)warp_pdf(w, f3((float)(sin_theta * cos_phi), (float)(sin_theta * sin_phi), (float)yy));
    };
    const double integral = adaptive_simpson_2d(integrand, y_start, x_start, y_end, x_end);
    q.exp[idx] = integral * q.scale;
    if (q.evals) q.evals[idx] = evals;
}

__global__ __launch_bounds__(64) void warp_query_kernel(WarpQuery q) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= q.n) return;
    const float a = q.in[3 * i], b = q.in[3 * i + 1], c = q.in[3 * i + 2];
    if (q.mode == NH_WARP_QUERY_PDF) {
        q.out[i] = warp_pdf(q.w, f3(a, b, c));
        return;
    }
    F3 p = f3(0, 0, 0);
    float weight = 0.f;
    switch (q.w.type) {
#define NH_WARP_CASE(T) case T: weight = warp_point<T>(q.w, a, b, c, p); break;
        NH_WARP_CASE(NH_WARP_NONE)
        NH_WARP_CASE(NH_WARP_DISK)
        NH_WARP_CASE(NH_WARP_UNIFORM_SPHERE)
        NH_WARP_CASE(NH_WARP_UNIFORM_SPHERE_VOL)
        NH_WARP_CASE(NH_WARP_UNIFORM_SPHERE_CAP)
        NH_WARP_CASE(NH_WARP_UNIFORM_HEMISPHERE)
        NH_WARP_CASE(NH_WARP_COSINE_HEMISPHERE)
        NH_WARP_CASE(NH_WARP_BECKMANN)
        NH_WARP_CASE(NH_WARP_HENYEY_GREENSTEIN)
        NH_WARP_CASE(NH_WARP_MICROFACET_BRDF)
        NH_WARP_CASE(NH_WARP_ISO_PHASE)
        NH_WARP_CASE(NH_WARP_ANISO_PHASE)
#undef NH_WARP_CASE
    }
    q.out[4 * i] = p.x;
    q.out[4 * i + 1] = p.y;
    q.out[4 * i + 2] = p.z;
    q.out[4 * i + 3] = weight;
}

namespace nh {

void launch_warp_histogram(const WarpHist &h, hipStream_t st) {
    if (h.n <= 0) return;
    const int64_t lanes = ((int64_t)h.n + h.run - 1) / h.run;
    const int groups = (int)((lanes + kChi2Block - 1) / kChi2Block);
    const size_t lds = ((size_t)h.xres * h.yres * (h.sub_tables ? kChi2Block / 64 : 1) + 1) * sizeof(uint32_t);
    hipLaunchKernelGGL(warp_histogram_kernel, dim3(groups), dim3(kChi2Block), lds, st, h);
}

void launch_warp_expected(const WarpExpected &e, hipStream_t st) {
    const int total = e.xres * e.yres;
    if (total <= 0) return;
    hipLaunchKernelGGL(warp_expected_kernel, dim3((total + 63) / 64), dim3(64), 0, st, e);
}

void launch_warp_query(const WarpQuery &q, hipStream_t st) {
    if (q.n <= 0) return;
    hipLaunchKernelGGL(warp_query_kernel, dim3((q.n + 63) / 64), dim3(64), 0, st, q);
}

}  // namespace nh
}  // namespace nh_disney
