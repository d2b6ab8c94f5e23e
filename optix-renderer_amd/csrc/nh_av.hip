// The av integrator (AverageVisibilityIntegrator, src/integrators/av.cpp) as a split pipeline: the stages of li_av
// (nh_integrators.h) around the context's batch traversal kernels (nh_kernels.hip launch_trace / launch_trace_wide),
// which it does not restate. DESIGN.md section 7f.
//
//   av_primary   one lane per (pixel, round) path: renderBlock's camera sample (render.cpp:441-447) exactly as
//                nh_path_kernel draws it, the camera ray into an SoA batch, the stream's state after the four draws.
//                It also clears the path's slot of the occlusion queue to a ray no traversal walks (maxt < mint).
//   (closest hits of the batch)
//   av_shade     a miss writes 1 into the path's sample record. A hit runs hit_info and the rejection sampler
//                (av_sample_hemisphere) and appends (its.p, dir, Epsilon, length) and its path index to the compact
//                occlusion queue: one ballot and one atomic per wave.
//   (any-hit queries of the queue: launched over the chunk's path count -- the entries past the queue's length are the
//    cleared ones, whole waves of which return at once -- so no grid is sized from the device counter)
//   av_resolve   entry j of the queue writes 0 (occluded) or 1 into the record of its path.
//
// The records then go through launch_splat like the megakernel's. No BSDF or emitter is evaluated: one build serves
// every scene.
#include "nh_integrators.h"

namespace {

constexpr int kAvBlock = 256;

__device__ __forceinline__ void av_record(float *rec, size_t r, float v) {
    rec[kRecFloats * r] = v;
    rec[kRecFloats * r + 1] = v;
    rec[kRecFloats * r + 2] = v;
}

__global__ __launch_bounds__(kAvBlock) void av_primary(const DScene *__restrict__ Sp, AvLaunch L) {
    const DScene &S = *Sp;
    const int gid = blockIdx.x * kAvBlock + threadIdx.x;
    if (gid >= L.n_paths) return;
    const int k = gid / L.n_list, i = gid - k * L.n_list;
    const int pix = L.pixel_list[i];
    const int py = pix / S.width, px = pix - py * S.width;
    const int sample = L.s0 + k;
    Rng rng = path_rng(L.seed, (uint64_t)pix, (uint64_t)sample);
    const float jx = rng.next1d(), jy = rng.next1d();
    rng.next1d();  // the aperture sample (render.cpp:443), unused
    rng.next1d();
    F3 o, d;
    float mint, maxt;
    camera_ray(S, (float)px + jx, (float)py + jy, o, d, mint, maxt, sample, pix);
    L.ray[0][gid] = o.x;
    L.ray[1][gid] = o.y;
    L.ray[2][gid] = o.z;
    L.ray[3][gid] = d.x;
    L.ray[4][gid] = d.y;
    L.ray[5][gid] = d.z;
    L.ray[6][gid] = mint;
    L.ray[7][gid] = maxt;
    L.rng[gid] = rng.state;
    // slot gid of the occlusion queue, until av_shade appends over it: maxt < mint, which every traversal returns on
    // before it reads the tree (nh_traverse.h); a finite direction, so nothing forms a NaN on the way there
    L.q_ray[0][gid] = 0.f;
    L.q_ray[1][gid] = 0.f;
    L.q_ray[2][gid] = 0.f;
    L.q_ray[3][gid] = 0.f;
    L.q_ray[4][gid] = 0.f;
    L.q_ray[5][gid] = 1.f;
    L.q_ray[6][gid] = 1.f;
    L.q_ray[7][gid] = 0.f;
}

__global__ __launch_bounds__(kAvBlock) void av_shade(const DScene *__restrict__ Sp, Traversal tv, AvLaunch L) {
    const DScene &S = *Sp;
    const int gid = blockIdx.x * kAvBlock + threadIdx.x;
    const bool live = gid < L.n_paths;
    bool hit = false;
    F3 p = f3(0, 0, 0), dir = f3(0, 0, 0);
    if (live) {
        if (L.hit.hit[gid]) {
            hit = true;
            Hit h;
            h.t = L.hit.t[gid];
            h.u = L.hit.u[gid];
            h.v = L.hit.v[gid];
            h.k = L.hit.k[gid];
            const F3 o = f3(L.ray[0][gid], L.ray[1][gid], L.ray[2][gid]);
            const F3 d = f3(L.ray[3][gid], L.ray[4][gid], L.ray[5][gid]);
            Its its;
            hit_info(S, tv, h, o, d, its);
            Rng rng;
            rng.state = L.rng[gid];
            rng.inc = ((uint64_t)(L.s0 + gid / L.n_list) << 1u) | 1u;  // path_rng's stream of the path's sample
            dir = av_sample_hemisphere(rng, its.sh.n);
            p = its.p;
        } else {
            av_record(L.rec, (size_t)gid, 1.f);
        }
    }
    // compact append: the wave's hits take consecutive slots from one atomic
    const unsigned long long mask = __ballot(hit);
    if (mask == 0ull) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)mask) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(L.q_count, (unsigned)__popcll(mask));
    base = __shfl(base, leader, 64);
    if (!hit) return;
    const unsigned j = base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));  // < n_paths: one slot per hit path
    L.q_ray[0][j] = p.x;
    L.q_ray[1][j] = p.y;
    L.q_ray[2][j] = p.z;
    L.q_ray[3][j] = dir.x;
    L.q_ray[4][j] = dir.y;
    L.q_ray[5][j] = dir.z;
    L.q_ray[6][j] = kEps;
    L.q_ray[7][j] = S.av_length;
    L.q_path[j] = gid;
}

__global__ __launch_bounds__(kAvBlock) void av_resolve(AvLaunch L) {
    const unsigned j = blockIdx.x * kAvBlock + threadIdx.x;
    if (j >= *L.q_count) return;
    av_record(L.rec, (size_t)L.q_path[j], L.q_hit[j] ? 0.f : 1.f);
}

}  // namespace

namespace nh {

void launch_av_primary(const DScene *S, const AvLaunch &L, hipStream_t st) {
    if (L.n_paths <= 0) return;
    hipLaunchKernelGGL(av_primary, dim3((L.n_paths + kAvBlock - 1) / kAvBlock), dim3(kAvBlock), 0, st, S, L);
}

void launch_av_shade(const DScene *S, const Traversal &tv, const AvLaunch &L, hipStream_t st) {
    if (L.n_paths <= 0) return;
    hipLaunchKernelGGL(av_shade, dim3((L.n_paths + kAvBlock - 1) / kAvBlock), dim3(kAvBlock), 0, st, S, tv, L);
}

void launch_av_resolve(const AvLaunch &L, int bound, hipStream_t st) {
    if (bound <= 0) return;
    hipLaunchKernelGGL(av_resolve, dim3((bound + kAvBlock - 1) / kAvBlock), dim3(kAvBlock), 0, st, L);
}

}  // namespace nh
