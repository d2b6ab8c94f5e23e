// The two tables of the reference's chi^2 test (src/utils/chi2test.cpp) on the device, over the bsdf_sample / bsdf_pdf
// device functions the render kernels call.
//
//   chi2_histogram_kernel   the sampling loop (chi2test.cpp:163-181). A lane owns a contiguous run of samples: one
//                           pcg_advance to its first draw, then sequential steps of the default-state pcg32. Counts go
//                           into a uint32 table in LDS with integer atomics -- one table per wave where four fit, so
//                           that waves do not meet on a narrow lobe's few cells -- and a workgroup's non-zero cells then
//                           into the global uint32 table, integer atomics again. Integer sums do not depend on arrival
//                           order: the same bits every run. No per-sample buffer, so n goes to INT32_MAX.
//   chi2_expected_kernel    the expected frequencies (chi2test.cpp:186-214): one lane per (wi, cell) runs
//                           adaptiveSimpson2D (nh_simpson.h) over the cell with the frames of both levels in private
//                           memory. About 10^4 pdf evaluations per test: throughput is not this kernel's business.
//
// Built once, with -DNH_DISNEY (Makefile), as nh_query.hip is: every BSDF type the HIP path has.
#include "nh_internal.h"
#include "nh_simpson.h"

#ifndef NH_DISNEY
#error "nh_chi2.hip is built with -DNH_DISNEY"
#endif

using namespace nhd;

namespace nh_disney {

namespace {
constexpr float kChi2InvTwoPi = 0.15915494309189533577f;  // INV_TWOPI (common.h)
constexpr float kChi2PiF = 3.14159265358979323846f;       // nori's M_PI is a float (common.h:61)

__device__ __forceinline__ int clamp_bin(int v, int res) { return min(max(0, v), res - 1); }
}  // namespace

__global__ __launch_bounds__(kChi2Block) void chi2_histogram_kernel(Chi2Hist h) {
    extern __shared__ uint32_t s_tab[];  // cells entries, or kChi2Block / 64 tables of them (sub_tables)
    const int cells = h.res_theta * h.res_phi;
    const int n_tab = h.sub_tables ? kChi2Block / 64 : 1;
    for (int i = threadIdx.x; i < n_tab * cells; i += kChi2Block) s_tab[i] = 0u;
    __syncthreads();
    uint32_t *tab = s_tab + (h.sub_tables ? (int)(threadIdx.x >> 6) * cells : 0);
    const int64_t lane = (int64_t)blockIdx.x * kChi2Block + threadIdx.x;
    const int64_t begin = lane * h.run;
    if (begin < (int64_t)h.n) {
        const int count = (int)min((int64_t)h.run, (int64_t)h.n - begin);
        const DBsdf b = h.bsdf;
        const F3 wi = f3(h.wi[0], h.wi[1], h.wi[2]), alb = f3(h.albedo[0], h.albedo[1], h.albedo[2]);
        Rng rng;
        rng.inc = kPcgDefaultStream;
        rng.state = pcg_advance(kPcgDefaultState, kPcgDefaultStream, h.first_draw + 2 * (uint64_t)begin);
        for (int k = 0; k < count; ++k) {
            // Point2f sample(random.nextFloat(), random.nextFloat()): x is the first draw, as nh_ttest_bsdf takes it
            const float sx = rng.next1d(), sy = rng.next1d();
            F3 wo;
            int measure = M_SOLID_ANGLE;
            const F3 w = bsdf_sample(b, wi, sx, sy, wo, measure, alb);
            if (w.x == 0.f && w.y == 0.f && w.z == 0.f) continue;  // (result.array() == 0).all()
            const int ct = clamp_bin((int)floorf((wo.z * 0.5f + 0.5f) * (float)h.res_theta), h.res_theta);
            float scaled_phi = f_atan2(wo.y, wo.x) * kChi2InvTwoPi;
            if (scaled_phi < 0.f) scaled_phi += 1.f;
            const int pb = clamp_bin((int)floorf(scaled_phi * (float)h.res_phi), h.res_phi);
            atomicAdd(&tab[ct * h.res_phi + pb], 1u);  // ct < res_theta and pb < res_phi: inside the table
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += kChi2Block) {
        uint32_t v = s_tab[i];
        for (int t = 1; t < n_tab; ++t) v += s_tab[t * cells + i];
        if (v) atomicAdd(&h.counts[i], v);
    }
}

__global__ __launch_bounds__(64) void chi2_expected_kernel(Chi2Expected q) {
    const int cells = q.res_theta * q.res_phi;
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= q.n_wi * cells) return;
    const int w = idx / cells, cell = idx - w * cells;
    const int i = cell / q.res_phi, j = cell - i * q.res_phi;
    const DBsdf b = q.bsdf;
    const F3 wi = f3(q.wi[3 * w], q.wi[3 * w + 1], q.wi[3 * w + 2]);
    // chi2test.cpp:190-194. cosThetaStart = -1.0 + i * 2.0 / res is fp64; phiStart = j * 2*M_PI / res is
    // ((float)(2 j) * M_PI) / (float)res in fp32, M_PI being a float, and widens afterwards
    const double cos_start = -1.0 + i * 2.0 / q.res_theta, cos_end = -1.0 + (i + 1) * 2.0 / q.res_theta;
    const double phi_start = (double)((float)(j * 2) * kChi2PiF / (float)q.res_phi);
    const double phi_end = (double)((float)((j + 1) * 2) * kChi2PiF / (float)q.res_phi);
    uint32_t evals = 0;
    const auto integrand = [&](double cos_theta, double phi) -> double {  // chi2test.cpp:196-206
        const double sin_theta = sqrt(1 - cos_theta * cos_theta);
        const double sin_phi = sin(phi), cos_phi = cos(phi);
        const F3 wo = f3((float)(sin_theta * cos_phi), (float)(sin_theta * sin_phi), (float)cos_theta);
        ++evals;
        return (double)bsdf_pdf(b, wi, wo, M_SOLID_ANGLE);
    };
    const double integral = adaptive_simpson_2d(integrand, cos_start, phi_start, cos_end, phi_end);
    q.exp[idx] = integral * (double)q.sample_count;
    if (q.evals) q.evals[idx] = evals;
}

namespace nh {

void launch_chi2_histogram(const Chi2Hist &h, hipStream_t st) {
    if (h.n <= 0) return;
    const int64_t lanes = ((int64_t)h.n + h.run - 1) / h.run;
    const int groups = (int)((lanes + kChi2Block - 1) / kChi2Block);
    const size_t lds = (size_t)h.res_theta * h.res_phi * (h.sub_tables ? kChi2Block / 64 : 1) * sizeof(uint32_t);
    hipLaunchKernelGGL(chi2_histogram_kernel, dim3(groups), dim3(kChi2Block), lds, st, h);
}

void launch_chi2_expected(const Chi2Expected &e, hipStream_t st) {
    const int total = e.n_wi * e.res_theta * e.res_phi;
    if (total <= 0) return;
    hipLaunchKernelGGL(chi2_expected_kernel, dim3((total + 63) / 64), dim3(64), 0, st, e);
}

}  // namespace nh
}  // namespace nh_disney
