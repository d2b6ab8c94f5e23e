// The reference's adaptive sampler on the HIP path: src/samplers/adaptive.cpp and the adaptive branch of
// renderThreadMain (src/utils/render.cpp:266, :323-336), in the reference's single-thread serial order (DESIGN.md
// section 7c). The image is cut into 4x4 blocks; within an outer sample every block renders pass after pass of
// size.x * size.y paths until its own variance test stops it. One pass of all the blocks still rendering is
//
//   ad_decide_kernel   per block: AdaptiveSampler::computeVariance on the block image the previous pass staged
//                      (computeVarianceFromImage, common.cpp:339-398; Eigen's sum() / squaredNorm() in the order of its
//                      linear vectorised redux; DiscretePDF), then either the block retires or getSampleIndices writes
//                      the pass's positions -- uniform, or drawn from the block's own pcg32 stream
//   ad_path_kernel     renderBlock's per-sample body over that explicit list: per-path stream, pixel jitter, camera
//                      ray and the integrator's Li (the li_* functions of nh_integrators.h, li_path_vol of nh_volume.h)
//   ad_put_kernel      ImageBlock::put(pos, value) of the pass's samples in list order into the block's own image, one
//                      64-lane wave per block, one lane per pixel of the (at most) 8x8 image, staged per (block, pass)
//
// and after the last pass of the outer sample
//
//   ad_merge_kernel    ImageBlock::put(block) into the master: per master pixel, the covering blocks in BlockGenerator
//                      spiral order, each block's passes in order -- fp32 sums do not commute, so nothing is pre-summed
//
// No kernel waits for another workgroup; the host reads one count per pass (the blocks still rendering).
//
// Built once, with -DNH_DISNEY (Makefile), as nh_volume.hip is: every BSDF and emitter type the HIP path has. The
// integrators are the device functions the megakernels call (nh_integrators.h, nh_volume.h).
#include "nh_dispatch.h"
#include "nh_integrators.h"
#include "nh_volume.h"

namespace nh_disney {

namespace {

constexpr float kAdEps = 1e-4f;  // Nori's Epsilon

// Color4f::divideByFilterWeight().getLuminance() (include/nori/color.h:113-118, common.cpp:265-268)
__device__ __forceinline__ float ad_luminance(float4 c) {
    float r = 0.f, g = 0.f, b = 0.f;
    if (fabsf(c.w) > kAdEps) { r = c.x / c.w; g = c.y / c.w; b = c.z / c.w; }
    return r * 0.212671f + g * 0.715160f + b * 0.072169f;
}

// Eigen 3.3.8's redux_impl<.., LinearVectorizedTraversal, NoUnrolling> (Eigen/src/Core/Redux.h) with scalar_sum_op
// over n coefficients in storage order, SSE2 Packet4f: packets from index 0, two accumulators over pairs of packets,
// accumulator 0 + accumulator 1, an odd last packet, predux (a0 + a2) + (a1 + a3), the remaining coefficients one by
// one; under 4 coefficients a left-to-right sum. Pinned to a recording (tests/golden/adaptive_eigen_redux.json).
__device__ float eigen_redux_sum(const float *v, int n) {
    const int aligned = n & ~3, aligned2 = n & ~7;
    if (aligned == 0) {
        float res = v[0];
        for (int i = 1; i < n; ++i) res += v[i];
        return res;
    }
    float p0[4] = {v[0], v[1], v[2], v[3]};
    if (aligned > 4) {
        float p1[4] = {v[4], v[5], v[6], v[7]};
        for (int i = 8; i < aligned2; i += 8)
            for (int l = 0; l < 4; ++l) {
                p0[l] += v[i + l];
                p1[l] += v[i + 4 + l];
            }
        for (int l = 0; l < 4; ++l) p0[l] += p1[l];
        if (aligned > aligned2)
            for (int l = 0; l < 4; ++l) p0[l] += v[aligned2 + l];
    }
    float res = (p0[0] + p0[2]) + (p0[1] + p0[3]);
    for (int i = aligned; i < n; ++i) res += v[i];
    return res;
}

}  // namespace

// AdaptiveSampler::computeVariance (adaptive.cpp:70-129) with the round render.cpp:326-334 hands it -- passes
// k = 0, 1, 2, 3, .. see rounds 0, 0, 1, 2, .. -- and getSampleIndices (adaptive.cpp:134-170). One lane per block.
__global__ __launch_bounds__(64) void ad_decide_kernel(AdaptiveLaunch A) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= A.n_blocks) return;
    AdBlock &st = A.state[r];
    if (A.k == 0) {
        st.active = 1;
        st.npass = 0;
        st.head = st.last = -1;
    }
    if (!st.active) return;
    const int4 blk = A.blocks[r];
    const int ox = blk.x, oy = blk.y, sx = blk.z, sy = blk.w, n = sx * sy, b = A.border;
    const int round = A.k == 0 ? 0 : A.k - 1;
    if (round == 0) {  // a new outer sample (and once more at pass 1)
        for (int i = 0; i < 16; ++i) st.old_var[i] = 0.f;
        st.old_norm = 10000.f;
    } else if (round == kAdMaxRound) {
        st.active = 0;
        return;
    }
    float cdf[17];
    bool adaptive = false;
    if (round >= A.initial_uniform) {
        adaptive = true;
        // computeVarianceFromImage (common.cpp:339-398) on the image the previous pass staged. std::pow(float, 2) is a
        // double pow and 1.f / sum a float: term and running sum in double, rounded to float once per term.
        const float4 *img = A.staging + (size_t)st.last * kAdImagePx;
        float lum[16], var[16];
        for (int i = 0; i < sy; ++i)
            for (int j = 0; j < sx; ++j) lum[i * 4 + j] = fabsf(ad_luminance(img[(i + b) * 8 + (j + b)]));
        float vmax = -INFINITY, vmin = INFINITY;
        for (int i = 0; i < sy; ++i)
            for (int j = 0; j < sx; ++j) {
                float mean = 0.f, sum = 0.f;
                for (int k = 0; k < 3; ++k)
                    for (int l = 0; l < 3; ++l) {
                        const int i_ = i - 1 + k, j_ = j - 1 + l;
                        if (i_ < 0 || i_ > sy - 1 || j_ < 0 || j_ > sx - 1) continue;
                        mean += lum[i_ * 4 + j_];
                        sum += 1.f;
                    }
                mean /= sum;
                const double inv = (double)(1.f / sum);
                float col = 0.f;
                for (int k = 0; k < 3; ++k)
                    for (int l = 0; l < 3; ++l) {
                        const int i_ = i - 1 + k, j_ = j - 1 + l;
                        if (i_ < 0 || i_ > sy - 1 || j_ < 0 || j_ > sx - 1) continue;
                        const double d = (double)(lum[i_ * 4 + j_] - mean);
                        col = (float)((double)col + inv * (d * d));
                    }
                var[i * 4 + j] = col;
                vmax = e_max(vmax, col);
                vmin = e_min(vmin, col);
            }
        const bool flat = vmax - vmin < kAdEps;
        for (int i = 0; i < sy; ++i)
            for (int j = 0; j < sx; ++j)
                var[i * 4 + j] = flat ? 0.f : 1.f + (var[i * 4 + j] - vmin) / (vmax - vmin) * 0.254f;
        // (m_oldVariance - variance).sum() and squaredNorm(): column-major coefficients of a size.y x size.x matrix
        float diff[16], sq[16];
        for (int j = 0; j < sx; ++j)
            for (int i = 0; i < sy; ++i) {
                diff[j * sy + i] = st.old_var[i * 4 + j] - var[i * 4 + j];
                sq[j * sy + i] = var[i * 4 + j] * var[i * 4 + j];
            }
        const float var_diff = fabsf(eigen_redux_sum(diff, n));
        // (the "one everywhere" exit of adaptive.cpp:98-103 cannot fire: the values are all 0, or span [1, 1.254])
        const float z = eigen_redux_sum(sq, n);  // variance.normalize(): a zero matrix stays as it is
        if (z > 0.f) {
            const float nz = f_sqrt(z);
            for (int i = 0; i < sy; ++i)
                for (int j = 0; j < sx; ++j) var[i * 4 + j] /= nz;
        }
        if (var_diff > st.old_norm) {  // stop improving this block
            st.active = 0;
            return;
        }
        st.old_norm = var_diff;
        for (int i = 0; i < sy; ++i)
            for (int j = 0; j < sx; ++j) st.old_var[i * 4 + j] = var[i * 4 + j];
        // DiscretePDF: append in row-major order, normalize (dpdf.h:55-57, :102-114)
        cdf[0] = 0.f;
        for (int i = 0; i < sy; ++i)
            for (int j = 0; j < sx; ++j) cdf[i * sx + j + 1] = cdf[i * sx + j] + var[i * 4 + j];
        const float total = cdf[n];
        if (total > 0.f) {
            const float norm = 1.0f / total;
            for (int i = 1; i <= n; ++i) cdf[i] *= norm;
            cdf[n] = 1.0f;
        }
    }
    // getSampleIndices: {i < size.y, j < size.x} or size.x * size.y draws; renderBlock reads the pair as (x, y)
    int2 *pos = A.pos + (size_t)r * kAdPaths;
    if (!adaptive) {
        for (int i = 0; i < sy; ++i)
            for (int j = 0; j < sx; ++j) pos[i * sx + j] = make_int2(i + ox, j + oy);
    } else {
        Rng rng;
        rng.state = st.rng_state;
        rng.inc = st.rng_inc;
        for (int m = 0; m < n; ++m) {
            const float u = rng.next1d();
            int idx = 0;  // std::lower_bound over the n + 1 CDF entries (dpdf.h:124-129)
            while (idx <= n && cdf[idx] < u) ++idx;
            int elem = idx - 1 < 0 ? 0 : idx - 1;
            elem = elem > n - 1 ? n - 1 : elem;
            pos[m] = make_int2(elem / sx + ox, elem % sx + oy);
        }
        st.rng_state = rng.state;
    }
    A.active_list[atomicAdd(&A.counts[A.k], 1u)] = r;
    atomicAdd(&A.stats[0], (unsigned long long)n);
    atomicAdd(&A.stats[1], 1ull);
    atomicMax(&A.stats[2], (unsigned long long)(A.k + 1));
}

// renderBlock (render.cpp:436-458) for sample i of an active block: the per-path stream of pixel index y W + x and
// sample index (s 1002 + k) 16 + i, two jitter draws, the unused aperture sample, then the integrator's draws. The
// surface integrators walk the tree left child first, the reference's order, whatever the request's traversal.
template <int DEPTH>
__global__ __launch_bounds__(64, 2) void ad_path_kernel(const DScene *__restrict__ Sp, Traversal tv, AdaptiveLaunch A) {
    __shared__ uint32_t stk[DEPTH * 64];
    const DScene &S = *Sp;
    const int gid = blockIdx.x * 64 + threadIdx.x;
    const int a = gid / kAdPaths, i = gid - a * kAdPaths;
    if (a >= A.n_active) return;
    const int r = A.active_list[a];
    const int4 blk = A.blocks[r];
    if (i >= blk.z * blk.w) return;
    const int2 p = A.pos[(size_t)r * kAdPaths + i];
    const int pix = p.y * S.width + p.x;
    const int sample = (A.s * kAdPassStride + A.k) * kAdPaths + i;
    Rng rng = path_rng(A.seed, (uint64_t)pix, (uint64_t)sample);
    const float jx = rng.next1d(), jy = rng.next1d();
    rng.next1d();
    rng.next1d();
    F3 o, d;
    float mint, maxt;
    camera_ray(S, (float)p.x + jx, (float)p.y + jy, o, d, mint, maxt, sample, pix);
    TravStats st{0, 0, 0};
    uint32_t queries = 0;
    uint32_t *sk = stk + threadIdx.x;
    F3 li;
    switch (S.integrator) {
        case 1: li = li_path_mats<DEPTH, false, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 2: li = li_direct_ems<DEPTH, false, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 3: li = li_direct_mats<DEPTH, false, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 4: li = li_direct_mis<DEPTH, false, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 5: li = li_direct_simple<DEPTH, false, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 6: li = li_normals<DEPTH, false, false>(S, tv, o, d, mint, maxt, sk, 64, st, queries); break;
        case 7: li = li_path_vol<DEPTH, false, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 8: li = li_path_vol<DEPTH, false, true>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 10: li = li_av<DEPTH, false, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
        case 11: li = li_envmaptester(S, d); break;
        default: li = li_path_mis<DEPTH, false, false>(S, tv, rng, o, d, mint, maxt, sk, 64, st, queries); break;
    }
    A.rad[gid] = make_float4(li.x, li.y, li.z, 0.f);
    A.jit[gid] = make_float2(jx, jy);
}

// ImageBlock::put(pos, value) (block.cpp:93-123) of the pass's samples, in list order, into the cleared block image.
// One wave per active block, lane (yt, xt) = one pixel of the array; every lane walks the same samples.
__global__ __launch_bounds__(64) void ad_put_kernel(AdaptiveLaunch A) {
    const int a = blockIdx.x, lane = threadIdx.x;
    const int r = A.active_list[a];
    const int4 blk = A.blocks[r];
    const int ox = blk.x, oy = blk.y, n = blk.z * blk.w, b = A.border;
    const int cols = blk.z + 2 * b, rows = blk.w + 2 * b;
    const int yt = lane >> 3, xt = lane & 7;
    float ar = 0.f, ag = 0.f, ab = 0.f, aw = 0.f;
    for (int i = 0; i < n; ++i) {
        const float4 v = A.rad[(size_t)a * kAdPaths + i];
        if (!is_valid(f3(v.x, v.y, v.z))) continue;  // an invalid sample drops with its weight
        const float2 j = A.jit[(size_t)a * kAdPaths + i];
        const int2 p = A.pos[(size_t)r * kAdPaths + i];
        const float px = ((float)p.x + j.x) - 0.5f - (float)(ox - b);
        const float py = ((float)p.y + j.y) - 0.5f - (float)(oy - b);
        const int x0 = max((int)ceilf(px - A.radius), 0), y0 = max((int)ceilf(py - A.radius), 0);
        const int x1 = min((int)floorf(px + A.radius), cols - 1), y1 = min((int)floorf(py + A.radius), rows - 1);
        if (xt < x0 || xt > x1 || yt < y0 || yt > y1) continue;
        const float wx = A.table[(int)(fabsf((float)xt - px) * A.lookup)];
        const float wy = A.table[(int)(fabsf((float)yt - py) * A.lookup)];
        ar += v.x * wx * wy;
        ag += v.y * wx * wy;
        ab += v.z * wx * wy;
        aw += 1.0f * wx * wy;
    }
    const int slot = A.slot_base + a;
    A.staging[(size_t)slot * kAdImagePx + lane] = make_float4(ar, ag, ab, aw);
    if (lane == 0) {
        AdBlock &st = A.state[r];
        if (st.last >= 0) A.next[st.last] = slot;
        else st.head = slot;
        st.last = slot;
        st.npass = A.k + 1;
    }
}

// m_block.put(block) (block.cpp:125-134) of every staged pass of the outer sample. One lane per master pixel: the
// blocks whose image covers it (two per axis at most) in spiral order, each block's passes in order, added to the
// master's value one after the other.
__global__ __launch_bounds__(256) void ad_merge_kernel(AdaptiveLaunch A) {
    const int mcols = A.width + 2 * A.border, mrows = A.height + 2 * A.border;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= mcols * mrows) return;
    const int Y = q / mcols, X = q - Y * mcols;
    int rank[4], off[4], cnt = 0;
    for (int by = Y / kAdBlock - 1; by <= Y / kAdBlock; ++by)
        for (int bx = X / kAdBlock - 1; bx <= X / kAdBlock; ++bx) {
            if (bx < 0 || by < 0 || bx >= A.nbx || by >= A.nby) continue;
            const int rk = A.block_rank[by * A.nbx + bx];
            const int4 blk = A.blocks[rk];
            const int lx = X - blk.x, ly = Y - blk.y;
            if (lx >= blk.z + 2 * A.border || ly >= blk.w + 2 * A.border) continue;
            int at = cnt++;
            while (at > 0 && rank[at - 1] > rk) {
                rank[at] = rank[at - 1];
                off[at] = off[at - 1];
                --at;
            }
            rank[at] = rk;
            off[at] = ly * 8 + lx;
        }
    float4 *fb = reinterpret_cast<float4 *>(A.fb);
    float4 acc = fb[q];
    bool any = false;
    for (int c = 0; c < cnt; ++c) {
        const AdBlock &st = A.state[rank[c]];
        int slot = st.head;
        for (int p = 0; p < st.npass; ++p) {
            const float4 v = A.staging[(size_t)slot * kAdImagePx + off[c]];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            if (p + 1 < st.npass) slot = A.next[slot];
            any = true;
        }
    }
    if (any) fb[q] = acc;
}

namespace nh {

void launch_adaptive_decide(const AdaptiveLaunch &A, hipStream_t st) {
    if (A.n_blocks <= 0) return;
    hipLaunchKernelGGL(ad_decide_kernel, dim3((A.n_blocks + 63) / 64), dim3(64), 0, st, A);
}

void launch_adaptive_paths(const DScene *S, const Traversal &tv, const AdaptiveLaunch &A, int depth, hipStream_t st) {
    if (A.n_active <= 0) return;
    const dim3 grid(((size_t)A.n_active * kAdPaths + 63) / 64);
    nh_dispatch_depth<32, 64, 128>(depth, [&](auto d) {
        hipLaunchKernelGGL((ad_path_kernel<d>), grid, dim3(64), 0, st, S, tv, A);
    });
}

void launch_adaptive_put(const AdaptiveLaunch &A, hipStream_t st) {
    if (A.n_active <= 0) return;
    hipLaunchKernelGGL(ad_put_kernel, dim3(A.n_active), dim3(64), 0, st, A);
}

void launch_adaptive_merge(const AdaptiveLaunch &A, hipStream_t st) {
    const int n = (A.width + 2 * A.border) * (A.height + 2 * A.border);
    hipLaunchKernelGGL(ad_merge_kernel, dim3((n + 255) / 256), dim3(256), 0, st, A);
}

}  // namespace nh
}  // namespace nh_disney
