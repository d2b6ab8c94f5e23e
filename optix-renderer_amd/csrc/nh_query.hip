// One path's radiance as a point query, and the reference's t-test estimators (src/utils/ttest.cpp) on the device.
//
//   path_query_kernel    one camera path per lane through the integrator's Li -- the li_* functions of
//                        nh_integrators.h and li_path_vol of nh_volume.h, the device functions the megakernels call.
//                        nh_radiance_query: sample s of pixel p on its per-path stream, as renderBlock draws it
//                        (render.cpp:441-447), the radiance as it is. nh_ttest_scene: sample k of StudentsTTest's scene
//                        loop (ttest.cpp:210-230) on the stream of (pixel 0, sample k), its luminance
//   ttest_bsdf_kernel    sample k of the BSDF loop (ttest.cpp:167-181) from draws 2k, 2k + 1 of the default-state pcg32
//   tt_partial_kernel,   the fp64 sum of the luminances, or of their squared deviations from a mean: per-lane strided
//   tt_final_kernel      sums, wave shuffles, one partial per workgroup, then one wave over the partials in index
//                        order. No atomics, and a launch geometry that depends on n alone: the same bits every run
//
// Built once, with -DNH_DISNEY (Makefile), as nh_volume.hip and nh_adaptive.hip are: every BSDF and emitter type the
// HIP path has.
#include "nh_dispatch.h"
#include "nh_integrators.h"
#include "nh_photon.h"
#include "nh_volume.h"

namespace nh_disney {

namespace {

// Color3f::getLuminance (include/nori/color.h)
__device__ __forceinline__ float tt_luminance(F3 c) { return c.x * 0.212671f + c.y * 0.715160f + c.z * 0.072169f; }

// lane 0 receives the sum of the wave's 64 values, added in a fixed tree
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

}  // namespace

// Closest hits nearer child first; every visit order returns the same hit.
template <int DEPTH>
__global__ __launch_bounds__(64, 2) void path_query_kernel(const DScene *__restrict__ Sp, Traversal tv, PathQuery q) {
    __shared__ uint32_t stk[DEPTH * 64];
    const DScene &S = *Sp;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= q.n) return;
    const bool ttest = q.lum != nullptr;
    const int pix = ttest ? 0 : q.pixel[i];
    const int sample = ttest ? 0 : q.sample[i];  // (its place in the lens stream: the t-test refuses a thin lens)
    Rng rng = path_rng(q.seed, (uint64_t)pix, ttest ? q.first + (uint64_t)i : (uint64_t)sample);
    const float jx = rng.next1d(), jy = rng.next1d();
    rng.next1d();  // the aperture sample (render.cpp:443, ttest.cpp:216), unused
    rng.next1d();
    float spx, spy;
    if (ttest) {  // sampler->next2D() * camera->getOutputSize().cast<float>() (ttest.cpp:214-215)
        spx = jx * (float)S.width;
        spy = jy * (float)S.height;
    } else if (q.pixel_sample) {
        spx = q.pixel_sample[i].x;
        spy = q.pixel_sample[i].y;
    } else {
        const int py = pix / S.width, px = pix - py * S.width;
        spx = (float)px + jx;
        spy = (float)py + jy;
    }
    F3 o, d;
    float mint, maxt;
    camera_ray(S, spx, spy, o, d, mint, maxt, sample, pix);
    TravStats st{0, 0, 0};
    uint32_t queries = 0;
    uint32_t *sk = stk + threadIdx.x;
    F3 li;
    switch (S.integrator) {
        case 1: li = li_path_mats<DEPTH, true, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 2: li = li_direct_ems<DEPTH, true, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 3: li = li_direct_mats<DEPTH, true, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 4: li = li_direct_mis<DEPTH, true, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 5: li = li_direct_simple<DEPTH, true, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 6: li = li_normals<DEPTH, true, false>(S, tv, o, d, mint, maxt, sk, 64, st, queries); break;
        case 7: li = li_path_vol<DEPTH, false, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 8: li = li_path_vol<DEPTH, false, true>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 9: li = li_photonmapper<DEPTH, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 10: li = li_av<DEPTH, true, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 11: li = li_envmaptester(S, d); break;
        default: li = li_path_mis<DEPTH, true, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
    }
    if (ttest) {
        q.lum[i] = tt_luminance(li);
    } else {
        q.rad[i] = make_float4(li.x, li.y, li.z, 0.f);
        if (q.jitter) q.jitter[i] = make_float2(jx, jy);
    }
}

// Point2f sample(random.nextFloat(), random.nextFloat()): x is the first draw, as the oracle's no_ttest_bsdf takes it
__global__ __launch_bounds__(64) void ttest_bsdf_kernel(BsdfTtest t) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= t.n) return;
    Rng rng;
    rng.inc = kPcgDefaultStream;
    rng.state = pcg_advance(kPcgDefaultState, kPcgDefaultStream, t.first_draw + 2 * (uint64_t)i);
    const float sx = rng.next1d(), sy = rng.next1d();
    F3 wo;
    int measure = M_SOLID_ANGLE;
    const F3 w = bsdf_sample(t.bsdf, f3(t.wi[0], t.wi[1], t.wi[2]), sx, sy, wo, measure,
                             f3(t.albedo[0], t.albedo[1], t.albedo[2]));
    t.lum[i] = tt_luminance(w);
}

// Workgroup b sums samples [b kTtPerBlock, (b + 1) kTtPerBlock): lane l takes l, l + kTtBlock, .. in that order
__global__ __launch_bounds__(kTtBlock) void tt_partial_kernel(const float *__restrict__ lum, int n, const double *center,
                                                              double *partial) {
    __shared__ double s_wave[kTtBlock / 64];
    const int base = blockIdx.x * kTtPerBlock;
    const double c = center ? *center : 0.0;
    double acc = 0.0;
    for (int j = threadIdx.x; j < kTtPerBlock; j += kTtBlock) {
        const int i = base + j;
        if (i >= n) break;
        double x = (double)lum[i];
        if (center) {
            x -= c;
            x *= x;
        }
        acc += x;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_wave[0];
        for (int w = 1; w < kTtBlock / 64; ++w) s += s_wave[w];
        partial[blockIdx.x] = s;
    }
}

// One wave: lane l sums partials l, l + 64, .. in that order
__global__ __launch_bounds__(64) void tt_final_kernel(const double *__restrict__ partial, int n_partial, double divisor,
                                                      double *out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += 64) acc += partial[i];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) *out = acc / divisor;
}

namespace nh {

void launch_path_query(const DScene *S, const Traversal &tv, const PathQuery &q, int depth, hipStream_t st) {
    if (q.n <= 0) return;
    const dim3 grid((q.n + 63) / 64);
    nh_dispatch_depth<32, 64, 128>(depth, [&](auto d) {
        hipLaunchKernelGGL((path_query_kernel<d>), grid, dim3(64), 0, st, S, tv, q);
    });
}

void launch_ttest_bsdf(const BsdfTtest &t, hipStream_t st) {
    if (t.n <= 0) return;
    hipLaunchKernelGGL(ttest_bsdf_kernel, dim3((t.n + 63) / 64), dim3(64), 0, st, t);
}

void launch_ttest_reduce(const float *lum, int n, const double *center, double divisor, double *partial, double *out,
                         hipStream_t st) {
    if (n <= 0) return;
    const int n_partial = (n + kTtPerBlock - 1) / kTtPerBlock;
    hipLaunchKernelGGL(tt_partial_kernel, dim3(n_partial), dim3(kTtBlock), 0, st, lum, n, center, partial);
    hipLaunchKernelGGL(tt_final_kernel, dim3(1), dim3(64), 0, st, partial, n_partial, divisor, out);
}

}  // namespace nh
}  // namespace nh_disney
