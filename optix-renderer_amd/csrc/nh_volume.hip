// Homogeneous participating media on the HIP path.
//
//   nh_vol_path_kernel   megakernel of the volumetric path tracers: one thread per (pixel, sample) camera path --
//                        renderBlock's per-pixel body + PathVolMATSIntegrator::Li / PathVolMISIntegrator::Li
//                        (li_path_vol, nh_volume.h), writing the sample records nh_path_kernel writes (the splat,
//                        chunking and sharding are shared)
//   medium_query_kernel  nh_medium_query: point queries of one medium through the device functions of nh_volume.h
//
// Built once, with -DNH_DISNEY (Makefile): every BSDF and emitter type the HIP path has (nh_device.h kDisney,
// kExtLights).
#include "nh_dispatch.h"
#include "nh_volume.h"

// waves per SIMD the register allocator must allow (profiles/volume_kernel_resources.txt)
#ifndef NH_VOL_WAVES
#define NH_VOL_WAVES 2
#endif

namespace nh_disney {

template <int BLOCK, int DEPTH, bool STATS, bool MIS>
__global__ __launch_bounds__(BLOCK, NH_VOL_WAVES) void nh_vol_path_kernel(const DScene *__restrict__ Sp, Traversal tv, PathLaunch L) {
    __shared__ uint32_t stk[DEPTH * BLOCK];
    const DScene &S = *Sp;
    const int gid = blockIdx.x * BLOCK + threadIdx.x;
    TravStats st{0, 0, 0};
    uint32_t queries = 0;
    if (gid < L.n_paths) {
        const int k = gid / L.n_list, i = gid - k * L.n_list;
        const int pix = L.pixel_list[i];
        const int py = pix / S.width, px = pix - py * S.width;
        const int sample = L.s0 + k;
        Rng rng = path_rng(L.seed, (uint64_t)pix, (uint64_t)sample);
        // renderBlock (render.cpp:441-447): pixel jitter, unused aperture sample
        const float jx = rng.next1d(), jy = rng.next1d();
        rng.next1d();
        rng.next1d();
        F3 o, d;
        float mint, maxt;
        camera_ray(S, (float)px + jx, (float)py + jy, o, d, mint, maxt, sample, pix);
        const F3 li = li_path_vol<DEPTH, STATS, MIS>(S, tv, rng, o, d, mint, maxt, stk + threadIdx.x, BLOCK, st, queries);
        const size_t r = (size_t)k * L.n_list + i;
        L.rec[kRecFloats * r] = li.x;
        L.rec[kRecFloats * r + 1] = li.y;
        L.rec[kRecFloats * r + 2] = li.z;
    }
    if (STATS) flush_stats(st, queries, stat_shard(L.counters));
}

// One thread per query
struct ArrayDraw {
    const float *u;
    int n;
    NHD float operator()() { return u[n++]; }
};
__global__ __launch_bounds__(64) void medium_query_kernel(const DScene *__restrict__ Sp, nh::MediumQuery q) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= q.n) return;
    const Medium m = medium_load(*Sp, q.medium + 1);
    if (q.mode == NH_MEDIUM_QUERY_FREE_PATH) {
        ArrayDraw draw{q.in + 2 * (size_t)i, 0};
        q.out[2 * (size_t)i] = medium_free_path(m, draw);
        q.out[2 * (size_t)i + 1] = (float)draw.n;
    } else if (q.mode == NH_MEDIUM_QUERY_TRANSMITTANCE) {
        const float *in = q.in + 6 * (size_t)i;
        const F3 tr = medium_transmittance(m, f3(in[0], in[1], in[2]), f3(in[3], in[4], in[5]));
        q.out[3 * (size_t)i] = tr.x;
        q.out[3 * (size_t)i + 1] = tr.y;
        q.out[3 * (size_t)i + 2] = tr.z;
    } else if (q.mode == NH_MEDIUM_QUERY_PHASE_SAMPLE) {
        const F3 wo = phase_sample(m, q.in[2 * (size_t)i], q.in[2 * (size_t)i + 1]);
        float *o = q.out + 4 * (size_t)i;
        o[0] = wo.x; o[1] = wo.y; o[2] = wo.z;
        o[3] = phase_pdf(m, wo);
    } else {
        const float *in = q.in + 3 * (size_t)i;
        q.out[i] = phase_pdf(m, f3(in[0], in[1], in[2]));
    }
}

namespace nh {

void launch_vol_path(const DScene *S, const Traversal &tv, const PathLaunch &L, bool mis, bool stats, int depth,
                     hipStream_t st) {
    if (L.n_paths <= 0) return;
    nh_dispatch_depth<32, 64, 128>(depth, [&](auto d) {
        constexpr int DEPTH = d, BLOCK = DEPTH <= 32 ? 128 : 64;
        const dim3 grid((L.n_paths + BLOCK - 1) / BLOCK);
        nh_dispatch([&](auto M, auto T) {
            hipLaunchKernelGGL((nh_vol_path_kernel<BLOCK, DEPTH, T, M>), grid, dim3(BLOCK), 0, st, S, tv, L);
        }, mis, stats);
    });
}

void launch_medium_query(const DScene *S, const MediumQuery &q, hipStream_t st) {
    if (q.n <= 0) return;
    hipLaunchKernelGGL(medium_query_kernel, dim3((q.n + 63) / 64), dim3(64), 0, st, S, q);
}

}  // namespace nh
}  // namespace nh_disney
