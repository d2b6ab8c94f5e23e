// The photon mapper's kernels (src/integrators/photonmapper.cpp).
//
//   photon_trace_kernel     PhotonMapper::preprocess: one photon path per lane on its own stream. Run twice per batch
//                           of paths with the same streams: a count pass (deposits per path), then, after an exclusive
//                           scan of the counts, a write pass that stores deposit j of path k at its place in (path,
//                           bounce) order. No atomics decide a photon's slot: the map is a function of the seed alone.
//   photon_keys_kernel      grid cell key of every deposit
//   photon_scatter_kernel   the sorted map: position, decoded direction and power in (cell key, deposit index) order;
//                           counts the occupied cells (an integer atomic: the count is order-independent)
//   nh_photon_path_kernel   megakernel of the camera pass: renderBlock's per-pixel body + PhotonMapper::Li, writing
//                           the sample records nh_path_kernel writes
//   photon_query_kernel     nh_photon_query: the codec and the gather as point queries
//
// The scan and the sort are hipcub's. Built once, with -DNH_DISNEY (Makefile).
#include <hipcub/hipcub.hpp>

#include "nh_dispatch.h"
#include "nh_photon.h"

namespace nh_disney {

template <int DEPTH, bool WRITE>
__global__ __launch_bounds__(64, 2) void photon_trace_kernel(const DScene *__restrict__ Sp, Traversal tv, PhotonTrace P) {
    __shared__ uint32_t stk[DEPTH * 64];
    const DScene &S = *Sp;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= P.n_paths) return;
    const uint64_t k = P.k0 + (uint64_t)i;
    if (!WRITE) {
        P.counts[i] = photon_path<DEPTH>(S, tv, P.seed, k, stk + threadIdx.x, 64, [](int, F3, F3, F3) {});
        return;
    }
    const long long first = P.base + P.offsets[i];
    long long slot = first;
    const int n = photon_path<DEPTH>(S, tv, P.seed, k, stk + threadIdx.x, 64, [&](int bounce, F3 p, F3 dir, F3 W) {
        if (slot < (long long)P.cap) {
            uint32_t tp, rgbe;
            pm_encode(dir, W, tp, rgbe);
            P.pos[3 * slot] = p.x;
            P.pos[3 * slot + 1] = p.y;
            P.pos[3 * slot + 2] = p.z;
            P.bytes[slot] = make_uint2(rgbe, tp);
            P.path[slot] = (uint32_t)k;
            P.bounce[slot] = bounce;
        }
        ++slot;
    });
    // m_emittedPhotons: the path that fills the map is the last one counted (exactly one path satisfies this)
    if (first < (long long)P.cap && first + n >= (long long)P.cap) *P.emitted = (int)(k + 1);
}

__global__ __launch_bounds__(256) void photon_keys_kernel(PhotonFinalize F) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F.n) return;
    F.keys[i] = pm_key_of(F.pm, f3(F.pos[3 * (size_t)i], F.pos[3 * (size_t)i + 1], F.pos[3 * (size_t)i + 2]));
    F.index[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void photon_scatter_kernel(PhotonFinalize F) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F.n) return;
    const size_t s = F.sorted_index[i];
    const uint2 b = F.bytes[s];
    const F3 d = pm_decode_dir(F.tab, b.y), w = pm_decode_power(F.tab, b.x);
    const_cast<float4 *>(F.pm.pos)[i] = make_float4(F.pos[3 * s], F.pos[3 * s + 1], F.pos[3 * s + 2], 0.f);
    const_cast<float4 *>(F.pm.dir)[i] = make_float4(d.x, d.y, d.z, 0.f);
    const_cast<float4 *>(F.pm.power)[i] = make_float4(w.x, w.y, w.z, 0.f);
    if (i == 0 || F.pm.keys[i] != F.pm.keys[i - 1]) atomicAdd(F.cells, 1ull);
}

#ifndef NH_PHOTON_WAVES
#define NH_PHOTON_WAVES 2
#endif
template <int BLOCK, int DEPTH, bool STATS>
__global__ __launch_bounds__(BLOCK, NH_PHOTON_WAVES) void nh_photon_path_kernel(const DScene *__restrict__ Sp, Traversal tv,
                                                                               PathLaunch L) {
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
        const F3 li = li_photonmapper<DEPTH, STATS>(S, tv, rng, o, d, mint, maxt, stk + threadIdx.x, BLOCK, st, queries);
        const size_t r = (size_t)k * L.n_list + i;
        L.rec[kRecFloats * r] = li.x;
        L.rec[kRecFloats * r + 1] = li.y;
        L.rec[kRecFloats * r + 2] = li.z;
    }
    if (STATS) flush_stats(st, queries, stat_shard(L.counters));
}

// One thread per query
__global__ __launch_bounds__(64) void photon_query_kernel(const DScene *__restrict__ Sp, PhotonQuery q) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= q.n) return;
    if (q.mode == NH_PHOTON_QUERY_CODEC) {
        const float *in = q.in + 6 * (size_t)i;
        uint32_t tp, rgbe;
        pm_encode(f3(in[0], in[1], in[2]), f3(in[3], in[4], in[5]), tp, rgbe);
        uint8_t *b = q.bytes + 6 * (size_t)i;
        b[0] = (uint8_t)(tp & 0xffu);
        b[1] = (uint8_t)(tp >> 8);
        b[2] = (uint8_t)(rgbe & 0xffu);
        b[3] = (uint8_t)((rgbe >> 8) & 0xffu);
        b[4] = (uint8_t)((rgbe >> 16) & 0xffu);
        b[5] = (uint8_t)(rgbe >> 24);
        const F3 d = pm_decode_dir(q.tab, tp), w = pm_decode_power(q.tab, rgbe);
        float *o = q.out + 6 * (size_t)i;
        o[0] = d.x; o[1] = d.y; o[2] = d.z;
        o[3] = w.x; o[4] = w.y; o[5] = w.z;
        return;
    }
    const DPhotonMap &pm = Sp->pm;
    F3 sum = f3(0, 0, 0);
    int count = 0;
    pm_gather(pm, f3(q.in[3 * (size_t)i], q.in[3 * (size_t)i + 1], q.in[3 * (size_t)i + 2]), [&](int j) {
        const float4 w = pm.power[j];
        sum = add(sum, f3(w.x, w.y, w.z));
        ++count;
    });
    q.count[i] = count;
    q.out[3 * (size_t)i] = sum.x;
    q.out[3 * (size_t)i + 1] = sum.y;
    q.out[3 * (size_t)i + 2] = sum.z;
}

namespace nh {

void launch_photon_trace(const DScene *S, const Traversal &tv, const PhotonTrace &P, int depth, hipStream_t st) {
    if (P.n_paths <= 0) return;
    const dim3 grid((P.n_paths + 63) / 64);
    nh_dispatch_depth<32, 64, 128>(depth, [&](auto d) {
        if (P.offsets) hipLaunchKernelGGL((photon_trace_kernel<d, true>), grid, dim3(64), 0, st, S, tv, P);
        else hipLaunchKernelGGL((photon_trace_kernel<d, false>), grid, dim3(64), 0, st, S, tv, P);
    });
}

size_t photon_scan_temp_bytes(int n) {
    size_t bytes = 0;
    const long long *in = nullptr;
    long long *out = nullptr;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, n, nullptr) != hipSuccess) return 0;
    return std::max<size_t>(bytes, 16);
}

hipError_t photon_scan(const long long *counts, long long *offsets, int n, void *tmp, size_t tmp_bytes, hipStream_t st) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, counts, offsets, n, st);
}

hipError_t photon_sort(const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *index_in, uint32_t *index_out,
                       int n, hipStream_t st) {
    size_t bytes = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, keys_in, keys_out, index_in, index_out, n, 0, 64, st);
    if (e != hipSuccess) return e;
    void *tmp = nullptr;
    if ((e = hipMalloc(&tmp, std::max<size_t>(bytes, 16))) != hipSuccess) return e;
    e = hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys_in, keys_out, index_in, index_out, n, 0, 64, st);
    const hipError_t s = hipStreamSynchronize(st);
    (void)hipFree(tmp);
    return e != hipSuccess ? e : s;
}

void launch_photon_keys(const PhotonFinalize &F, hipStream_t st) {
    if (F.n <= 0) return;
    hipLaunchKernelGGL(photon_keys_kernel, dim3((F.n + 255) / 256), dim3(256), 0, st, F);
}

void launch_photon_scatter(const PhotonFinalize &F, hipStream_t st) {
    if (F.n <= 0) return;
    hipLaunchKernelGGL(photon_scatter_kernel, dim3((F.n + 255) / 256), dim3(256), 0, st, F);
}

void launch_photon_path(const DScene *S, const Traversal &tv, const PathLaunch &L, bool stats, int depth, hipStream_t st) {
    if (L.n_paths <= 0) return;
    nh_dispatch_depth<32, 64, 128>(depth, [&](auto d) {
        constexpr int DEPTH = d, BLOCK = DEPTH <= 32 ? 128 : 64;
        const dim3 grid((L.n_paths + BLOCK - 1) / BLOCK);
        nh_dispatch([&](auto T) {
            hipLaunchKernelGGL((nh_photon_path_kernel<BLOCK, DEPTH, T>), grid, dim3(BLOCK), 0, st, S, tv, L);
        }, stats);
    });
}

void launch_photon_query(const DScene *S, const PhotonQuery &q, hipStream_t st) {
    if (q.n <= 0) return;
    hipLaunchKernelGGL(photon_query_kernel, dim3((q.n + 63) / 64), dim3(64), 0, st, S, q);
}

}  // namespace nh
}  // namespace nh_disney
