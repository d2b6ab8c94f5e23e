// gfx950 kernels of the path_mis hot path.
//
//   nh_trace_kernel   BVH::rayIntersect over an SoA ray batch (parity entry point)
//   nh_path_kernel    megakernel: one thread per (pixel, sample) camera path --
//                     renderBlock's per-pixel body + the integrator's Li (nh_integrators.h: PathMISIntegrator::Li,
//                     PathMatsIntegrator::Li, the direct integrators; src/utils/render.cpp:436-458,
//                     src/integrators/path_mis.cpp:16-150, path_mats.cpp:16-78), writing (radiance, jitter) sample
//                     records
//   (the ImageBlock stage -- splat and merge of the sample records -- is in nh_splat.hip)
#include <cstdlib>
#include <type_traits>

#ifndef NH_DEFAULT_PATH_WAVES
#define NH_DEFAULT_PATH_WAVES 4
#endif
#include "nh_dispatch.h"
#include "nh_integrators.h"

// Built a second time with -DNH_DISNEY (Makefile): the same kernels and launchers with the Disney branch of the BSDF
// functions compiled in (nh_device.h kDisney), as nh_disney::nh::launch_* (nh_internal.h)
#ifdef NH_DISNEY
namespace nh_disney {
#endif

template <int BLOCK, int DEPTH, bool ORDERED, bool ANY, bool STATS>
__global__ __launch_bounds__(BLOCK) void nh_trace_kernel(const DScene *__restrict__ Sp, Traversal tv, RayBatch rb,
                                                         HitBatch hb, int n, unsigned long long *counters) {
    __shared__ uint32_t stk[DEPTH * BLOCK];
    const DScene &S = *Sp;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    TravStats st{0, 0, 0};
    if (i < n) {
        F3 o = f3(rb.ox[i], rb.oy[i], rb.oz[i]), d = f3(rb.dx[i], rb.dy[i], rb.dz[i]);
        Hit h;
        bool hit = trace<DEPTH, ORDERED, ANY, STATS>(tv, S, o, d, rb.mint[i], rb.maxt[i], h, stk + threadIdx.x, BLOCK, st);
        hb.hit[i] = hit ? 1 : 0;
        if (!ANY) {
            hb.t[i] = hit ? h.t : INFINITY;
            hb.u[i] = hit ? h.u : 0.f;
            hb.v[i] = hit ? h.v : 0.f;
            hb.k[i] = hit ? h.k : -1;
        }
    }
    if (STATS) flush_stats(st, i < n ? 1u : 0u, stat_shard(counters));
}

// The same entry point over the 4-wide (or 8-wide, W = 8) collapse (nh_traverse.h Tracer4 / Tracer8), run to
// completion per lane: LDS window of 16 (ref, distance) entries, deeper entries in the lane's `spill` area.
template <bool ORDERED, bool ANY, bool STATS, int W = 4>
__global__ __launch_bounds__(64) void nh_trace_wide_kernel(const DScene *__restrict__ Sp, Traversal tv, RayBatch rb,
                                                           HitBatch hb, int n, int2 *spill, int spill_depth,
                                                           unsigned long long *counters) {
    __shared__ int s_ref[16 * 64];
    __shared__ float s_near[16 * 64];
    const DScene &S = *Sp;
    const int i = blockIdx.x * 64 + threadIdx.x;
    TravStats st{0, 0, 0};
    if (i < n) {
        RingStack2<16> stk{s_ref + threadIdx.x, s_near + threadIdx.x, 64, spill, (unsigned)n, (unsigned)i};
        typename std::conditional<W == 8, Tracer8<ORDERED, ANY, STATS, RingStack2<16>>,
                                  Tracer4<ORDERED, ANY, STATS, RingStack2<16>>>::type tr;
        tr.begin(S, tv, f3(rb.ox[i], rb.oy[i], rb.oz[i]), f3(rb.dx[i], rb.dy[i], rb.dz[i]), rb.mint[i], rb.maxt[i], st);
        while (!tr.done) tr.step(tv, stk, st);
        hb.hit[i] = tr.found ? 1 : 0;
        if (!ANY) {
            hb.t[i] = tr.found ? tr.best.t : INFINITY;
            hb.u[i] = tr.found ? tr.best.u : 0.f;
            hb.v[i] = tr.found ? tr.best.v : 0.f;
            hb.k[i] = tr.found ? tr.best.k : -1;
        }
    }
    if (STATS) flush_stats(st, i < n ? 1u : 0u, stat_shard(counters));
}

// PM: a path_mis scene without normal maps -- only li_path_mis, normal maps compiled out. The kernel with every
// integrator (and hit_info's normal-map calls) holds registers and code that cost the path_mis megakernel 6 %
// (profiles/round6_ab_nmap.txt).
template <int BLOCK, int DEPTH, bool ORDERED, bool STATS, int MINW, bool PM = false>
__global__ __launch_bounds__(BLOCK, MINW) void nh_path_kernel(const DScene *__restrict__ Sp, Traversal tv, PathLaunch L) {
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
        const float spx = (float)px + jx, spy = (float)py + jy;
        F3 o, d;
        float mint, maxt;
        camera_ray(S, spx, spy, o, d, mint, maxt, sample, pix);
        F3 li;
        if (PM) li = li_path_mis<DEPTH, ORDERED, STATS, false>(S, tv, rng, o, d, mint, maxt, stk + threadIdx.x, BLOCK, st, queries);
        else switch (S.integrator) {
            case 1: li = li_path_mats<DEPTH, ORDERED, STATS>(S, tv, rng, o, d, mint, maxt, stk + threadIdx.x, BLOCK, st, queries); break;
            case 2: li = li_direct_ems<DEPTH, ORDERED, STATS>(S, tv, rng, o, d, mint, maxt, stk + threadIdx.x, BLOCK, st, queries); break;
            case 3: li = li_direct_mats<DEPTH, ORDERED, STATS>(S, tv, rng, o, d, mint, maxt, stk + threadIdx.x, BLOCK, st, queries); break;
            case 4: li = li_direct_mis<DEPTH, ORDERED, STATS>(S, tv, rng, o, d, mint, maxt, stk + threadIdx.x, BLOCK, st, queries); break;
            case 5: li = li_direct_simple<DEPTH, ORDERED, STATS>(S, tv, rng, o, d, mint, maxt, stk + threadIdx.x, BLOCK, st, queries); break;
            case 6: li = li_normals<DEPTH, ORDERED, STATS>(S, tv, o, d, mint, maxt, stk + threadIdx.x, BLOCK, st, queries); break;
            case 10: li = li_av<DEPTH, ORDERED, STATS>(S, tv, rng, o, d, mint, maxt, stk + threadIdx.x, BLOCK, st, queries); break;
            case 11: li = li_envmaptester(S, d); break;
            default: li = li_path_mis<DEPTH, ORDERED, STATS>(S, tv, rng, o, d, mint, maxt, stk + threadIdx.x, BLOCK, st, queries); break;
        }
        const size_t r = (size_t)k * L.n_list + i;
        L.rec[kRecFloats * r] = li.x;
        L.rec[kRecFloats * r + 1] = li.y;
        L.rec[kRecFloats * r + 2] = li.z;
    }
    if (STATS) flush_stats(st, queries, stat_shard(L.counters));
}

// ---------------------------------------------------------------------------
// host-side launchers (called from nh_api.hip and nh_pipeline.hip)
// ---------------------------------------------------------------------------
namespace nh {

#ifndef NH_DISNEY  // the traversal entry points have no Disney copy
void launch_trace(const DScene *S, const Traversal &tv, const RayBatch &rb, const HitBatch &hb, int n, bool any,
                  bool ordered, bool stats, int depth, unsigned long long *ctr, hipStream_t st) {
    if (n <= 0) return;
    nh_dispatch_depth<16, 32, 64, 128>(depth, [&](auto d) {
        constexpr int DEPTH = d, BLOCK = DEPTH <= 32 ? 128 : 64;
        const dim3 grid((n + BLOCK - 1) / BLOCK);
        nh_dispatch([&](auto O, auto A, auto T) {
            hipLaunchKernelGGL((nh_trace_kernel<BLOCK, DEPTH, O, A, T>), grid, dim3(BLOCK), 0, st, S, tv, rb, hb, n, ctr);
        }, ordered, any, stats);
    });
}

void launch_trace_wide(const DScene *S, const Traversal &tv, const RayBatch &rb, const HitBatch &hb, int n, bool any,
                       bool ordered, bool stats, int2 *spill, int spill_depth, unsigned long long *ctr,
                       hipStream_t st, int wide) {
    if (n <= 0) return;
    dim3 grid((n + 63) / 64);
    nh_dispatch([&](auto O, auto A, auto T) {
        if (wide == 8) hipLaunchKernelGGL((nh_trace_wide_kernel<O, A, T, 8>), grid, dim3(64), 0, st, S, tv, rb, hb, n,
                                          spill, spill_depth, ctr);
        else hipLaunchKernelGGL((nh_trace_wide_kernel<O, A, T>), grid, dim3(64), 0, st, S, tv, rb, hb, n, spill,
                                spill_depth, ctr);
    }, ordered, any, stats);
}
#endif

// occupancy target of the megakernel (waves per SIMD the register allocator must allow)
static int path_min_waves() {
    static int w = [] {
        const char *e = std::getenv("NH_PATH_WAVES");
        int v = e ? std::atoi(e) : NH_DEFAULT_PATH_WAVES;
        return (v >= 1 && v <= 4) ? v : NH_DEFAULT_PATH_WAVES;
    }();
    return w;
}

void launch_path(const DScene *S, const Traversal &tv, const PathLaunch &L, bool ordered, bool stats, int depth,
                 bool pm, hipStream_t st) {
    if (L.n_paths <= 0) return;
    nh_dispatch_depth<16, 32, 64, 128>(depth, [&](auto d) {
        constexpr int DEPTH = d, BLOCK = DEPTH <= 32 ? 128 : 64;
        const dim3 grid((L.n_paths + BLOCK - 1) / BLOCK);
        const auto launch = [&](auto w) {
            constexpr int MINW = w;
            const auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(BLOCK), 0, st, S, tv, L); };
            // the PM kernel is built for near-first traversal only: a left-first request takes the full kernel
            if (ordered && pm) nh_dispatch([&](auto T) { go(nh_path_kernel<BLOCK, DEPTH, true, T, MINW, true>); }, stats);
            else nh_dispatch([&](auto O, auto T) { go(nh_path_kernel<BLOCK, DEPTH, O, T, MINW>); }, ordered, stats);
        };
        // 4 waves/SIMD measured best (13.7 / 13.8 / 9.8 / 8.3 ms per 16M C2 samples at 1 / 2 / 3 / 4);
        // the 2-wave build stays selectable (NH_PATH_WAVES=2) for register-heavy experiments
        // deep stacks (DEPTH > 32) are LDS-limited below 4 waves anyway: build them for 2
        if constexpr (DEPTH > 32) {
            launch(std::integral_constant<int, 2>{});
        } else {
            if (path_min_waves() == 2) launch(std::integral_constant<int, 2>{});
            else launch(std::integral_constant<int, 4>{});
        }
    });
}

}  // namespace nh

#ifdef NH_DISNEY
}  // namespace nh_disney
#endif
