// Internal structures shared between the C-ABI layer (nh_api.hip, nh_upload.hip, nh_pipeline.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nh_device.h"
#include "nh_traverse.h"
#include "nori_hip.h"

struct RayBatch {
    const float *ox, *oy, *oz, *dx, *dy, *dz, *mint, *maxt;
};
struct HitBatch {
    uint8_t *hit;
    float *t, *u, *v;
    int *k;
};
// floats per sample record: (r, g, b), padded to 4 with NH_REC_STRIDE=4 (16-B aligned records, an A/B build)
#ifndef NH_REC_STRIDE
#define NH_REC_STRIDE 3
#endif
constexpr int kRecFloats = NH_REC_STRIDE;

struct PathLaunch {
    int n_paths;            // n_rounds * n_list
    int n_list;             // pixels rendered by this context
    int s0;                 // first sample round of the chunk
    uint64_t seed;
    const int *pixel_list;  // y*W+x per list entry (ordered block by block)
    float *rec;             // (r, g, b) per (round, list entry); the splat recomputes the pixel jitter (sample_jitter)
    unsigned long long *counters;
};
// One chunk of the av integrator's split pipeline (nh_av.hip): n_paths = rounds * n_list paths, path r = round k, list
// entry i at k * n_list + i like PathLaunch's records. Every array holds n_paths entries.
struct AvLaunch {
    int n_paths, n_list, s0;
    uint64_t seed;
    const int *pixel_list;
    float *rec;        // the chunk's sample records
    float *ray[8];     // camera rays, SoA in RayBatch's order (ox, oy, oz, dx, dy, dz, mint, maxt)
    HitBatch hit;      // their closest hits
    uint64_t *rng;     // pcg32 state of the path's stream after the four camera draws (inc follows from the sample)
    float *q_ray[8];   // the compact occlusion queue, the same order; entries past *q_count are rays with maxt < mint
    int *q_path;       // path of queue entry j
    uint8_t *q_hit;    // its any-hit result
    unsigned *q_count; // entries appended (zero before av_shade)
};
// Row pitch (float4) of one (round, block) ImageBlock of (32+2b)^2 pixels in the splat's staging buffer: rows start
// on 128-B lines, so the merge's 16-pixel row segments (master columns 16a..16a+15 = block columns 0..15 / 16..31)
// read whole lines instead of straddling three (the unpadded 36-float4 rows start 64 B off a line every other row)
__host__ __device__ __forceinline__ int stage_pitch(int cols) { return (cols + 7) & ~7; }
// Offset (float4) of block-array pixel (xt, yt) in one (round, block) ImageBlock of the staging buffer (stride
// cols * stage_pitch(cols)). band = 1 (the 36x36 arrays of the tabulated splat): the 32x32 core row-major, then the
// right band (columns 32..35, 36 rows of 4), then the bottom band (rows 32..35, 32 columns), so the merge's reads --
// a wave's 4 rows x 16 master columns of one block's core, or of a neighbour's band -- are whole 128-B lines
__host__ __device__ __forceinline__ int stage_off(int cols, int band, int xt, int yt) {
    if (!band) return yt * stage_pitch(cols) + xt;
    if (xt >= 32) return 1024 + yt * 4 + (xt - 32);
    if (yt >= 32) return 1024 + 144 + (yt - 32) * 32 + xt;
    return yt * 32 + xt;
}

struct SplatLaunch {
    float *fb;              // master RGBW (W+2b)x(H+2b)
    int width, height, border, reach, nbx, n_rounds, n_list;
    const int *pixel_map;   // image pixel -> list entry or -1
    const int *block_rank;  // BlockGenerator spiral rank per block id
    const float *rec;       // (r, g, b) per (round, list entry)
    const float2 *jit;      // the stored jitter per record (A/B knob), else null: recomputed
    uint64_t seed;          // the chunk's seed and first sample round: the jitter of round k's sample at pixel p is
    int s0;                 // sample_jitter(seed, p, s0 + k), the camera sample's first two draws
    float radius, lookup;
    float table[33];
    // block-local ImageBlocks (one per (round, rendered block)), (32+2b)^2 RGBW each
    const int *blocks;      // rendered block ids, slot order
    const int *block_slot;  // block id -> slot or -1
    int n_blocks;
    float4 *staging;
    int staged;             // 1: staged pair (splat into staging, then merge); 0: the fused tile splat (no staging).
                            // Fixed when the chunk's staging was sized, so a knob change mid-pipeline cannot
                            // mismatch the two
    int direct;             // rounds the tab splat added to fb for pixels one block covers (the merge starts them there)
    int persist;            // tab splat: a grid of this many workgroups walks the items (0: one workgroup per item)
    int band;               // staging offsets: stage_off(.., band, ..) (1: the tabulated splat's core + band layout)
    const int *color_slots; // slots of the blocks with (bx + by) even, then odd: the pair splat's two launches
    int n_color0;           // how many are even
    int debug;              // timing experiments only (NH_SPLAT_DEBUG, images wrong): bits skip the fused splat's
                            // phase 1 (1), phase 2 (2), record fetch (4), master-border strips (8)
};

// SimpleDenoiser pass (nh_denoise.hip): interior pixel (i, j) of an image at ptr[i * stride + j]
struct DenoiseLaunch {
    const float4 *src;      // the image at the start of the pass
    int src_stride;
    float4 *dst;            // the denoised image (pixels before p in row-major order already final)
    int dst_stride;
    int width, height, range;
    float sigma_vr;
    const float *g;         // g_sigma by squared pixel distance, 2 range^2 + 1 entries (host expf)
    float *var;             // raw variance per pixel (width * height)
    unsigned *minmax;       // [0] max, [1] min of var (float bits)
    int band_first;         // band of workgroup 0 of this launch
    int lag;                // launches between a band's chunk k and the next band's chunk k
    int chunk;              // wavefront steps per band per launch
};

// In-kernel work counters (collect_stats): kStatShards copies of [0-3] queries, nodes, boxes, prims,
// [4] invalid samples, [8-11] the any-hit share, [16-19] / [20-23] the closest / any-hit work of
// the tail kernel, one copy per XCD (workgroup b adds to copy b % 8) so the per-wave atomics of
// concurrent workgroups do not serialise on one address.
constexpr int kStatShards = 8, kStatStride = 48, kStatAny = 8, kStatTail = 16, kStatTailAny = 20;
// wf_tail_rr calibration clocks: 4 phase cycle sums, path-bounces, longest chain (max over shards)
constexpr int kStatTailClk = 24;
constexpr int kStatTailCoopClk = 32;  // [32-35] the same phases for bounces carried by lane groups, [36] their count
// wf_bounce_rr calibration clocks: [40-45] cycle sums of its phases (load, body, shadow, closest, head, store),
// [46] the path-bounces it ran
constexpr int kStatBounceClk = 40;
__device__ __forceinline__ unsigned long long *stat_shard(unsigned long long *c) {
    return c + (blockIdx.x & (kStatShards - 1)) * kStatStride;
}
// a kernel's closest / any-hit work into counters[0-3] (the megakernels: nh_kernels.hip, nh_volume.hip)
__device__ __forceinline__ void flush_stats(const nhd::TravStats &st, uint32_t queries, unsigned long long *counters) {
    // one atomic per wave: reduce over the 64 lanes first
    unsigned long long v[4] = {queries, st.nodes, st.boxes, st.prims};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned long long x = v[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&counters[i], x);
    }
}

namespace nh {
void launch_trace(const nhd::DScene *S, const nhd::Traversal &tv, const RayBatch &rb, const HitBatch &hb, int n,
                  bool any, bool ordered, bool stats, int depth, unsigned long long *ctr, hipStream_t st);
void launch_trace_wide(const nhd::DScene *S, const nhd::Traversal &tv, const RayBatch &rb, const HitBatch &hb, int n,
                       bool any, bool ordered, bool stats, int2 *spill, int spill_depth, unsigned long long *ctr,
                       hipStream_t st, int wide = 4);
// pm: a path_mis scene without normal maps (the kernel instantiation with only li_path_mis and no normal maps)
void launch_path(const nhd::DScene *S, const nhd::Traversal &tv, const PathLaunch &L, bool ordered, bool stats,
                 int depth, bool pm, hipStream_t st);
void launch_splat(const SplatLaunch &P, hipStream_t st);
// the av integrator's stages around the batch traversals above (nh_av.hip); bound: queue entries to resolve at most
void launch_av_primary(const nhd::DScene *S, const AvLaunch &L, hipStream_t st);
void launch_av_shade(const nhd::DScene *S, const nhd::Traversal &tv, const AvLaunch &L, hipStream_t st);
void launch_av_resolve(const AvLaunch &L, int bound, hipStream_t st);
// false: launch_splat adds the records straight into the master (no per-(round, block) staging buffer)
bool splat_uses_staging(int border, int reach);
void launch_count_invalid(const float *rec, size_t n, unsigned long long *out, hipStream_t st);
void launch_denoise_variance(const DenoiseLaunch &P, hipStream_t st);
int denoise_band_rows();
int denoise_max_chunk();
int tree_top_nodes();  // wide nodes the persistent traversal stages in LDS (nh_wavefront.hip)
size_t denoise_tile_static_lds();
// tile_bytes > 0: the LDS-tiled kernel with that much dynamic shared memory (both windows of a chunk)
void launch_denoise_band(const DenoiseLaunch &P, int L, int n_bands, size_t tile_bytes, hipStream_t st);
void launch_denoise_copy(const float4 *src, int src_stride, float4 *dst, int dst_stride, int width, int height,
                         hipStream_t st);
}  // namespace nh

// Queue appends go to one counter per XCD (blocks are dealt round-robin over the 8 XCDs), so no
// address takes device-scope atomics from more than one XCD.
constexpr int kQueueShards = 8, kCountStride = 32;

// Wavefront path state (nh_wavefront.hip): one side of the double-buffered, dense SoA state.
// Slot s of a buffer holds one live path; pid is its sample-record index (round * n_list + entry).
struct WfBuf {
    float4 *ray_o;           // (origin, pdf of the BSDF sample that made the ray); mint = Epsilon
    float4 *ray_d;           // (direction, flags << kPidBits | pid); maxt = +inf, -inf for d = 0
    float4 *hit;             // (t, u, v, prim index bits or -1) from the extend kernel
    uint64_t *rng;           // pcg32 state (inc is derived from the sample index)
    float4 *li;              // (Li, w_mats)
    float4 *thr;             // (throughput, w_ems if the queued shadow ray is occluded)
    float4 *pend;            // queued NEE: (w_ems * t * Li_ems, w_ems if unoccluded)
    uint8_t *occl;           // any-hit result of the path's shadow ray
};
struct WfState {
    WfBuf buf[2];
    float4 *sh_o, *sh_d;     // shadow queue: (origin, mint), (direction, maxt)
    int *sh_slot;            // slot of the shadow ray's path in the buffer shade wrote
    unsigned *counts;        // per-shard append counters, one 128-B line each:
                             // [s * kCountStride] paths, [(kQueueShards + s) * kCountStride] shadow rays
};
// Queue counts live on the device: the shade kernel of bounce i appends into count slot
// (i+1)&1, the kernels of bounce i+1 read it (8 shard counts -> dense prefix) -- the host never
// sizes a grid from them, it only reads them back (one bounce behind) to know when to stop.
// A count slot holds 4 groups of kQueueShards counters, each on its own 128-B line:
//   group 0 path appends, 1 shadow-ray appends, 2 / 3 persistent extend / any-hit fetch cursors.
constexpr int kCountGroup = kQueueShards * kCountStride;
constexpr int kCountSlot = 4 * kCountGroup;

struct WfLaunch {
    WfState st;
    int n_paths, n_list, s0;
    uint64_t seed;
    const int *pixel_list;
    float *rec;             // (r, g, b) per (round, list entry)
    float2 *jit;            // NH_SPLAT_JITTER=stored only: the jitter per record, written at the first vertex
    int in_q;               // buffer (and count slot) read by this bounce
    int first;              // bounce 0: paths come from the camera, not from a buffer
    int cam_rays;           // bounce 0 of a thin-lens scene on the persistent kernels: the camera rays were written raw
                            // into buf[in_q].ray_o / ray_d by wf_camera_rays (the persistent refill builds pinhole
                            // rays only)
    unsigned *cnt_in;       // count slot of this bounce's input queues
    unsigned *cnt_out;      // count slot the shade kernel appends into
    int seg_cap;            // entries per shard segment of every queue / buffer
    // small scenes: float4 / int2 counts of the BVH arrays staged into LDS by the traversal
    // kernels (0 = traverse from HBM)
    int small_nodes, small_leaves, small_prims;
    int small_frames;  // 1: the fused kernels also stage the flat triangles' shading frames (Traversal::frames)
    // The LDS image of a small scene, built once per upload (nh_upload.hip build_small_image): float4 regions in this
    // order -- nodes, primitive records, leaf table, pair records, pair-leaf table, scene tables, flat-triangle frames -- which the
    // fused kernels copy as it stands (stage_small_scene). small_tab: float4 counts of the table regions (shapes,
    // bsdfs, emitters, the emitting meshes' area CDFs, emit_faces), all 0 when the tables are not staged (over
    // kSmallTablesBytes, or a scene the diffuse area-light kernels do not run on): only those kernels read them.
    const float4 *small_image;
    int small_tab[5];
    // persistent traversal: per-lane stack spill area (kPersistentBlocks * 128 lanes x spill_depth
    // 32-bit words; the 4-wide traversal spills (ref, distance) pairs)
    uint32_t *trav_spill;
    int spill_depth;
    unsigned long long *counters;
    // Candidate masks of the camera rays' first closest hit (host/primary_masks.cpp), one per 32x32 block of the image's
    // block grid (by * nbx + bx; nbx = pmask_nbx), bit k = primitive record k; null: every record is tested. Read by
    // first_vertex of the non-STATS fused bounce kernels only.
    const unsigned long long *pmask;
    int pmask_nbx;
    // Candidate masks of the light sample's any-hit query at bounce 0 (host/shadow_masks.cpp), indexed as pmask; null:
    // every record is tested. Read by rr_step of the non-STATS wf_bounce_rr kernels that run bounce 0.
    const unsigned long long *smask;
    // The flat image of a scene whose tree is one leaf or a root with two leaves (nh_layout.h kFlatHeaderF4), or null:
    // the non-STATS wf_bounce_rr kernels are launched in their FLAT instantiation with it (trace_flat).
    const float4 *flat;
};
// persistent traversal grid: 16 workgroups of 128 lanes per CU (the 8 waves/SIMD its registers allow)
constexpr int kPersistentBlocks = 256 * 16;
constexpr size_t kSmallSceneBytes = 16384;
constexpr int kSmallFramesMaxPrims = 256;  // frames staged (48 B per record) only for scenes this small
// LDS budget of the scene tables staged beside a small BVH (shapes 64 B, BSDFs 48 B, emitters 32 B each, the emitting
// meshes' area CDFs, 48 B per emitting face): the Cornell box needs under 1 KB; 4 KB keeps four bounce workgroups
// per CU (each 16 KB of stacks + the scene copy) inside the CU's 160 KB
constexpr size_t kSmallTablesBytes = NH_SMALL_TABLES_BYTES;
namespace nh {
void launch_wf_trace(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool ordered, bool stats,
                     bool shadow, bool persistent, int wide, int bound, int depth, hipStream_t st);
// sort: entries shaded in the order of their hit's BSDF type within each workgroup (material-sorted shading)
// closest-hit + any-hit queries of a bounce in one persistent launch (4-wide tree); bound = both queues' sum
void launch_wf_trace2(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool ordered, bool stats,
                      int wide, int bound, hipStream_t st);
// bounce 0 of a thin-lens scene on the persistent kernels: every camera ray (camera_ray with its lens sample) into
// buf[in_q].ray_o / ray_d, (origin, mint) / (direction, maxt), for the persistent refill to read (WfLaunch::cam_rays)
void launch_wf_camera_rays(const nhd::DScene *S, const WfLaunch &L, int bound, hipStream_t st);
void launch_wf_shade(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool sort, bool nmap, int bound,
                     hipStream_t st);
// fused shade + any-hit + closest-hit bounce for LDS-staged BVHs; sort = material-sorted output queue
void launch_wf_bounce(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool ordered, bool stats,
                      bool sort, int bound, hipStream_t st);
// RR-ahead variants of the fused bounce / tail (nh_wavefront.hip): the stored state is a path after its
// vertex's Russian roulette
// lean: the FULL = false body (no mirror / dielectric BSDF, no texture); nmap: the scene has shape normal maps (else the
// full body is the NMAP = false instantiation)
// trait: the scene qualifies for the diffuse area-light instantiations (launch_wf_bounce_trait / launch_wf_tail_trait),
// taken when the other arguments allow them (near-first traversal, unsorted queue, the lean 2-wave tail)
void launch_wf_bounce_rr(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool ordered, bool stats, bool sort,
                         bool lean, bool nmap, bool trait, int bound, hipStream_t st);
void launch_wf_tail_rr(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool ordered, bool stats, int bound,
                       bool specular, bool lean, bool nmap, bool trait, hipStream_t st);
// wf_bounce_rr / wf_tail_rr<.., TRAIT = true>: near-first traversal, unsorted queue; bounce 0 (L.first) and the later
// bounces are separate instantiations. Their own translation-unit part of nh_wavefront.hip.
void launch_wf_bounce_trait(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool stats, int bound,
                            hipStream_t st);
void launch_wf_tail_trait(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool stats, int bound,
                          int coop, hipStream_t st);
void launch_wf_tail(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool ordered, bool stats,
                    int wide, int bound, int depth, hipStream_t st);
// copies the live RR-ahead paths of L's input queue (at most bound) densely into dst, count into dst_counts[0]
void launch_wf_pack_rr(const WfLaunch &L, const WfBuf &dst, unsigned *dst_counts, int bound, hipStream_t st);
// n_copy count words src -> host_dst (pinned, device-visible), then n_zero words of zero cleared (wf_counts_kernel)
// the computed regions of a small scene's LDS image (pair records at float4 pairs_off, frames at frames_off or none
// if < 0), from n_prim_f4 / 3 primitive records, by the float operations the kernels' own staging used to run; slots
// (device): the two records of each pair position (host/gpu_layout.cpp pair_layout)
void launch_small_image(const nhd::Traversal &tv, int n_prim_f4, const int2 *slots, int pairs_off, int frames_off,
                        float4 *image, hipStream_t st);
void launch_wf_counts(const unsigned *src, unsigned *host_dst, int n_copy, unsigned *zero, int n_zero, hipStream_t st);
}  // namespace nh

// The Disney variant (nh_device.h kDisney). nh_kernels.hip and nh_wavefront.hip are compiled a second time with
// -DNH_DISNEY, which puts everything they define into namespace nh_disney: the same kernels with the Disney branch of
// bsdf_eval / bsdf_pdf / bsdf_sample compiled in. nh_upload_scene chooses the set (nh_ctx::disney): a scene without a
// Disney BSDF launches exactly the nh:: kernels it always did. Only the launchers whose kernels shade are declared.
namespace nh_disney {
namespace nh {
void launch_path(const nhd::DScene *S, const nhd::Traversal &tv, const PathLaunch &L, bool ordered, bool stats,
                 int depth, bool pm, hipStream_t st);
void launch_wf_shade(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool sort, bool nmap, int bound,
                     hipStream_t st);
void launch_wf_bounce(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool ordered, bool stats,
                      bool sort, int bound, hipStream_t st);
void launch_wf_bounce_rr(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool ordered, bool stats, bool sort,
                         bool lean, bool nmap, bool trait, int bound, hipStream_t st);
void launch_wf_tail_rr(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool ordered, bool stats, int bound,
                       bool specular, bool lean, bool nmap, bool trait, hipStream_t st);
void launch_wf_tail(const nhd::DScene *S, const nhd::Traversal &tv, const WfLaunch &L, bool ordered, bool stats,
                    int wide, int bound, int depth, hipStream_t st);
// nh_disney.hip. The direction-independent scalars and the constant-albedo colour terms of n DDisney records
// (albedo: 3 floats per record), by the device functions eval uses for a textured albedo
void launch_disney_fold(nhd::DDisney *recs, const float *albedo, int n, hipStream_t st);
// nh_bsdf_query's kernel: bsdf_eval + bsdf_pdf (mode 0) or bsdf_sample + bsdf_pdf (mode 1) of one DBsdf, n queries
struct BsdfQuery {
    nhd::DBsdf bsdf;
    float albedo[3];
    int mode, n;
    const float *wi, *wo, *sample;
    float *wo_out, *value, *pdf;
    int *measure;
};
void launch_bsdf_query(const BsdfQuery &q, hipStream_t st);
// nh_emitter_query's kernel (nh_emitter_query.hip): emitter_sample (mode 0), emitter_eval (1) or emitter_pdf (2) of
// S.emitters[emitter], n queries. in: 2 floats per query (mode 0: the sample) or NH_EMITTER_QUERY_IN_STRIDE (wi, p, n);
// out: NH_EMITTER_QUERY_SAMPLE_STRIDE, 3 or 1 floats per query
struct EmitterQuery {
    int emitter, mode, n;
    const float *ref, *in;
    float *out;
};
void launch_emitter_query(const nhd::DScene *S, const EmitterQuery &q, hipStream_t st);
// nh_volume.hip. The volumetric path tracers (path_vol_mats / path_vol_mis: S->integrator 7 / 8), one thread per
// (pixel, round) like launch_path, writing the same sample records; built once, with every BSDF and emitter type.
// The closest hits are walked nearer child first whatever the request's traversal (every order returns the same hit).
void launch_vol_path(const nhd::DScene *S, const nhd::Traversal &tv, const PathLaunch &L, bool mis, bool stats, int depth,
                     hipStream_t st);
// nh_medium_query's kernel: medium_free_path (mode 0), medium_transmittance (1), phase_sample + phase_pdf (2) or
// phase_pdf (3) of S.media[medium], n queries. in / out: 2 / 2, 6 / 3, 2 / 4, 3 / 1 floats per query
struct MediumQuery {
    int medium, mode, n;
    const float *in;
    float *out;
};
void launch_medium_query(const nhd::DScene *S, const MediumQuery &q, hipStream_t st);
}  // namespace nh
}  // namespace nh_disney

// ---- the photon mapper (nh_photon.hip, driven by nh_photon_api.hip) ----
// One launch of the photon pass over paths k0 .. k0 + n_paths - 1. Count pass (offsets == null): counts[i] = deposits
// of path k0 + i, without a cap. Write pass: deposit j of path k0 + i goes to slot base + offsets[i] + j if that is
// below cap, and the path whose deposits reach slot cap - 1 writes *emitted = its index + 1.
struct PhotonTrace {
    uint64_t seed, k0;
    int n_paths;
    long long *counts;
    const long long *offsets;  // exclusive prefix sums of counts
    long long base;            // deposits of the paths before k0
    int cap;                   // photonCount
    float *pos;                // deposit order: 3 floats per photon
    uint2 *bytes;              // (rgbe[0..3], theta | phi << 8)
    uint32_t *path;
    int *bounce;
    int *emitted;
};
// the sorted map from the deposit-order arrays: keys of the deposits, then (after the sort of (key, index)) the sorted
// records with direction and power decoded through `tab`, and the number of distinct keys
struct PhotonFinalize {
    int n;
    const float *pos;
    const uint2 *bytes;
    const float *tab;
    nhd::DPhotonMap pm;  // origin, cell set; pos / dir / power / keys point at the sorted arrays to fill
    uint64_t *keys;      // unsorted keys (deposit order)
    uint32_t *index;     // 0 .. n - 1
    const uint32_t *sorted_index;
    unsigned long long *cells;
};
// nh_photon_query's kernel: mode 0 the codec (in: 6 floats, bytes: 6, out: 6 floats), mode 1 the gather (in: 3 floats,
// count: 1, out: 3 floats)
struct PhotonQuery {
    int mode, n;
    const float *in;
    const float *tab;
    uint8_t *bytes;
    int *count;
    float *out;
};
namespace nh_disney {
namespace nh {
void launch_photon_trace(const nhd::DScene *S, const nhd::Traversal &tv, const PhotonTrace &P, int depth, hipStream_t st);
// exclusive prefix sums (hipcub::DeviceScan), enqueued on st. tmp: photon_scan_temp_bytes(n_max) bytes, n <= n_max
size_t photon_scan_temp_bytes(int n);
hipError_t photon_scan(const long long *counts, long long *offsets, int n, void *tmp, size_t tmp_bytes, hipStream_t st);
void launch_photon_keys(const PhotonFinalize &F, hipStream_t st);
// stable radix sort of (key, index) pairs by key (hipcub::DeviceRadixSort): equal keys keep their deposit order
hipError_t photon_sort(const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *index_in, uint32_t *index_out,
                       int n, hipStream_t st);
void launch_photon_scatter(const PhotonFinalize &F, hipStream_t st);
// the camera pass: one thread per (pixel, round) like launch_vol_path, PhotonMapper::Li, the same sample records
void launch_photon_path(const nhd::DScene *S, const nhd::Traversal &tv, const PathLaunch &L, bool stats, int depth,
                        hipStream_t st);
void launch_photon_query(const nhd::DScene *S, const PhotonQuery &q, hipStream_t st);
}  // namespace nh
}  // namespace nh_disney

// ---- the adaptive sampler's render loop (nh_adaptive.hip, driven by nh_adaptive_api.hip) ----
constexpr int kAdBlock = 4;          // NORI_BLOCK_SIZE_ADAPTIVE (block.h:31)
constexpr int kAdPaths = 16;         // paths of a pass of a full block
constexpr int kAdPassStride = 1002;  // sample indices per outer sample: (s * 1002 + pass) * 16 + i
constexpr int kAdMaxRound = 1000;    // adaptive.cpp:78
constexpr int kAdMaxBorder = 2;      // a block image is at most 8 x 8: one lane per pixel in the put kernel
constexpr int kAdImagePx = 64;       // float4 entries of one staged (block, pass) image, row pitch 8
// One block's AdaptiveSampler clone plus the chain of its staged passes of the outer sample in flight
struct AdBlock {
    uint64_t rng_state, rng_inc;  // m_random: seed(offset.x, offset.y) once, then only the index draws
    float old_var[16];            // m_oldVariance, entry (i, j) at i * 4 + j
    float old_norm;               // m_oldNorm
    int active;                   // still rendering passes of this outer sample
    int npass;                    // passes staged this outer sample
    int head, last;               // first / latest staging slot of those passes (AdaptiveLaunch::next chains them)
    int pad;
};
struct AdaptiveLaunch {
    int n_blocks, nbx, nby;       // 4x4 blocks, indexed by BlockGenerator spiral rank below
    int width, height, border, initial_uniform;
    int s, k;                     // outer sample, pass
    uint64_t seed;
    const int4 *blocks;           // (offset x, offset y, size x, size y) by rank
    const int *block_rank;        // rank of block id by * nbx + bx
    AdBlock *state;               // by rank
    int *active_list;             // ranks of the blocks rendering pass k, in no particular order
    unsigned *counts;             // [pass]: blocks rendering it (the host reads one per pass)
    int n_active;                 // counts[k], as the host read it (path, put)
    int2 *pos;                    // [rank * 16 + i]: the chosen positions of pass k, image coordinates
    float4 *rad;                  // [active index * 16 + i]: (r, g, b, -) of path i
    float2 *jit;                  // its pixel jitter
    float4 *staging;              // kAdImagePx entries per slot
    int *next;                    // slot -> the slot of the same block's next pass
    int slot_base;                // slot of active index 0 of pass k
    unsigned long long *stats;    // [0] samples placed, [1] passes, [2] the most passes of a block in an outer sample
    float *fb;                    // master RGBW
    float radius, lookup;
    float table[33];
};
namespace nh_disney {
namespace nh {
// the variance test of pass k per block (AdaptiveSampler::computeVariance) and, for the blocks that go on, the pass's
// positions (getSampleIndices)
void launch_adaptive_decide(const AdaptiveLaunch &A, hipStream_t st);
// renderBlock's per-sample body over the explicit position list: the integrator's Li, built with every BSDF and
// emitter type; closest hits nearer child first whatever the request's traversal
void launch_adaptive_paths(const nhd::DScene *S, const nhd::Traversal &tv, const AdaptiveLaunch &A, int depth, hipStream_t st);
// ImageBlock::put of the pass's samples in list order into one staged image per active block
void launch_adaptive_put(const AdaptiveLaunch &A, hipStream_t st);
// m_block.put(block) of every staged pass of the outer sample, per master pixel in the serial order
void launch_adaptive_merge(const AdaptiveLaunch &A, hipStream_t st);
}  // namespace nh
}  // namespace nh_disney

// ---- the per-path radiance query and the t-test estimators (nh_query.hip, driven by nh_query_api.hip) ----
// One camera path per lane, for nh_radiance_query (lum == null: entry i = sample sample[i] of pixel pixel[i];
// pixel_sample / jitter may be null) and for the scene branch of StudentsTTest (lum != null: entry j = sample
// first + j of pixel 0 through (a W, b H), its luminance into lum[j]; the arrays are not read)
struct PathQuery {
    uint64_t seed;
    int n;
    const int *pixel, *sample;
    const float2 *pixel_sample;
    float4 *rad;   // (r, g, b, -)
    float2 *jitter;
    uint64_t first;
    float *lum;
};
// The BSDF branch of StudentsTTest: sample j takes draws first_draw + 2j, + 2j + 1 of the default-state pcg32
struct BsdfTtest {
    uint64_t first_draw;
    int n;
    nhd::DBsdf bsdf;
    float albedo[3], wi[3];
    float *lum;
};
constexpr int kTtBlock = 256;      // lanes of a reduction workgroup
constexpr int kTtPerBlock = 4096;  // samples one workgroup reduces: the partial count depends on n alone
namespace nh_disney {
namespace nh {
// built with every BSDF and emitter type; closest hits nearer child first
void launch_path_query(const nhd::DScene *S, const nhd::Traversal &tv, const PathQuery &q, int depth, hipStream_t st);
void launch_ttest_bsdf(const BsdfTtest &t, hipStream_t st);
// fp64 sum over j < n of lum[j] (center == null) or (lum[j] - *center)^2, divided by `divisor`, into *out: per-lane
// strided sums, wave shuffles, one partial per workgroup of kTtPerBlock samples (partial: (n + kTtPerBlock - 1) /
// kTtPerBlock doubles), then one wave over the partials in index order. No atomics: the same n gives the same bits.
void launch_ttest_reduce(const float *lum, int n, const double *center, double divisor, double *partial, double *out,
                         hipStream_t st);
}  // namespace nh
}  // namespace nh_disney

// ---- the chi^2 test's two tables (nh_chi2.hip, driven by nh_chi2_api.hip) ----
// ChiSquareTest's sampling loop: lane l owns samples [l run, (l + 1) run) of the n, sample j at draws first_draw + 2j,
// + 2j + 1 of the default-state pcg32. counts: res_theta * res_phi uint32, zeroed by the caller
struct Chi2Hist {
    uint64_t first_draw;
    int n, run;
    int res_theta, res_phi;
    int sub_tables;  // 1: every wave of a workgroup counts into its own LDS table (kChi2Block / 64 of them fit)
    nhd::DBsdf bsdf;
    float albedo[3], wi[3];
    uint32_t *counts;
};
// The expected frequencies: entry w * cells + cell of exp / evals is cell `cell` of incident direction wi[3w..3w + 2]
struct Chi2Expected {
    int n_wi, res_theta, res_phi, sample_count;
    nhd::DBsdf bsdf;
    const float *wi;
    double *exp;
    uint32_t *evals;  // may be null
};
constexpr int kChi2Block = 256;        // lanes of a histogram workgroup
constexpr int kChi2MinRun = 16;        // fewest samples a lane owns: one pcg_advance per run
constexpr int kChi2MaxGroups = 2048;   // most workgroups of a histogram launch; beyond it the runs grow
namespace nh_disney {
namespace nh {
void launch_chi2_histogram(const Chi2Hist &h, hipStream_t st);
void launch_chi2_expected(const Chi2Expected &e, hipStream_t st);
}  // namespace nh
}  // namespace nh_disney

// ---- the warp test (warptest.cpp's runTest; nh_warp.hip, driven by nh_warp_api.hip) ----
// What every warp kernel knows of the test: the NH_WARP_* type, the mapped parameter, and for the microfacet BRDF the
// incident direction and the BSDF record (alpha = parameter, kd = 0)
struct WarpSpec {
    int type;
    float parameter;
    float wi[3];
    nhd::DBsdf bsdf;
};
// generatePoints + the binning loop: lane l owns points [l run, (l + 1) run) of the n, point j at draws first_draw + 3j
// .. + 3j + 2 of the default-state pcg32 (rtl: x is the last of the three). counts: yres * xres uint32 and *nan_points,
// zeroed by the caller. The block size, run length and grid cap are the chi^2 histogram's (kChi2Block, ..)
struct WarpHist {
    WarpSpec w;
    uint64_t first_draw;
    int n, run;
    int xres, yres;
    int rtl;
    int sub_tables;
    uint32_t *counts;
    uint32_t *nan_points;
};
struct WarpExpected {
    WarpSpec w;
    int xres, yres;
    double scale;  // sample_count x 1, 4 or 4 * M_PI
    double *exp;
    uint32_t *evals;  // may be null
};
// one lane per query: mode NH_WARP_QUERY_SAMPLE (in 3n, out 4n) or NH_WARP_QUERY_PDF (in 3n, out n)
struct WarpQuery {
    WarpSpec w;
    int mode, n;
    const float *in;
    float *out;
};
namespace nh_disney {
namespace nh {
void launch_warp_histogram(const WarpHist &h, hipStream_t st);
void launch_warp_expected(const WarpExpected &e, hipStream_t st);
void launch_warp_query(const WarpQuery &q, hipStream_t st);
}  // namespace nh
}  // namespace nh_disney
