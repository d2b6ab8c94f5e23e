// The context behind the C-ABI (include/nori_hip.h) and what its three translation units share: nh_api.hip (create /
// destroy, ray queries, results, denoise, reduce), nh_upload.hip (scene and BVH upload) and nh_pipeline.hip (nh_render
// and the wavefront pipeline). Private to those three.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdint>
#include <deque>
#include <memory>
#include <string>
#include <vector>

#include "nh_internal.h"
#include "nori_hip.h"

// ---- wavefront pipeline state (nh_pipeline.hip) ----
constexpr int kRing = 4;   // bounce-count copies in flight per pool
// path pools in flight: while one drains its last bounces (long specular chains are a latency chain of
// hundreds of bounces) the next ones fill the GPU; NH_POOLS=1..kPools overrides the default (2 measured
// best: C4 2134-2147 Msamples/s vs 1913-1938 at 3 pools and 2078-2092 at 4; C2 / bumpy-1M unchanged)
constexpr int kPools = 4;
// tail slots: a chunk whose last live paths were handed off (RR-ahead pipeline, several pools) finishes its tail
// kernel and splat on one of these (own stream, small packed path buffer), while its pool takes the next chunk
constexpr int kTails = 3;
constexpr int kTailCap = 65536;  // paths a tail slot holds (the fused bounce's tail threshold is at most this)
#ifndef NH_DEFAULT_POOLS
#define NH_DEFAULT_POOLS 2
#endif

// one chunk of sample rounds of one nh_render call
struct WfJob {
    uint64_t seq;  // submission order = splat order
    int s0, rounds;
    uint64_t seed;
    bool ordered, stats;
    bool staged;   // splat layout, decided once when the chunk's buffers are sized (NH_SPLAT_FUSED read then only):
                   // per-(round, block) staging + merge, or the fused tile splat with no staging
    bool jit;      // NH_SPLAT_JITTER=stored (A/B): the first vertex stores each sample's jitter for the splat
};

// A path pool: the device state one chunk needs (double-buffered path state, shadow queue, sample
// records, block ImageBlocks, traversal spill area) plus its own stream, events and pinned
// count ring, and the host-side state machine of the chunk it is running.
struct WfPool {
    hipStream_t stream = nullptr;
    WfState wf{};
    std::vector<void *> bufs;
    size_t cap = 0;  // paths
    float *rec = nullptr;  // (r, g, b) per sample
    size_t rec_cap = 0;
    float2 *jit = nullptr;  // stored jitter (NH_SPLAT_JITTER=stored only)
    size_t jit_cap = 0;
    float4 *staging = nullptr;
    size_t staging_cap = 0;
    uint32_t *spill = nullptr;
    int spill_words = 0;
    unsigned *h_counts = nullptr;  // pinned: kRing bounce-count copies + one initial count slot
    hipEvent_t copy_ev[kRing] = {};
    std::vector<hipEvent_t> events;  // 4 per bounce (timing)
    hipEvent_t ev_begin = nullptr, ev_path = nullptr, ev_splat0 = nullptr, ev_splat = nullptr;
    hipEvent_t ev_handoff = nullptr;  // the packed tail paths are written (a tail slot's stream waits for it)
    enum State { IDLE, ENQUEUE, COUNTS, SPLAT, FINISH } state = IDLE;
    WfJob job{};
    WfLaunch L{};
    bool persistent = false, wide = false, trace2 = false, tail = false, draining = false;
    bool fused = false, sorted = false;  // one wf_bounce kernel per bounce (LDS-staged BVH); material-sorted queue
    bool rr = false;                     // fused kernels with the next vertex's Russian roulette ahead (wf_bounce_rr)
    bool trait = false;                  // RR-ahead kernels' diffuse area-light instantiations (nh_ctx::diffuse_area)
    bool shade_sorted = false;           // wf_shade entries in BSDF-type order (deep BVHs, mixed materials)
    int64_t tail_at = 0, drain_at = 0;
    int it = 0;
    std::vector<uint64_t> in_e, in_s;  // live paths / shadow rays entering each bounce
};

// RCCL communicators of one set of contexts (nh_reduce_framebuffers), created once and reused while the
// same contexts (by creation id, in the same order) reduce again; destroyed with the last holder.
struct CommSet {
    std::vector<uint64_t> ids;  // nh_ctx::id of the members, in rank order
    std::vector<int> devices;
    std::vector<ncclComm_t> comms;
    ~CommSet() {
        int cur = 0;
        const bool have = hipGetDevice(&cur) == hipSuccess;
        for (size_t i = 0; i < comms.size(); ++i) {
            (void)hipSetDevice(devices[i]);
            (void)ncclCommDestroy(comms[i]);
        }
        if (have) (void)hipSetDevice(cur);  // leave the caller's thread on its own device
    }
};

// restores the calling thread's current device when an entry point that walks several devices returns
struct DeviceGuard {
    int dev = 0;
    bool ok = false;
    DeviceGuard() { ok = hipGetDevice(&dev) == hipSuccess; }
    ~DeviceGuard() {
        if (ok) (void)hipSetDevice(dev);
    }
};

// The pixels a context renders (nh_render_req::blocks; all blocks by default) and the splat's block tables, built as
// a whole by ensure_pixel_list (nh_pipeline.hip): a context's list is always complete or absent
struct PixelList {
    int *pixel_list = nullptr, *pixel_map = nullptr;
    int *block_ids = nullptr, *block_slot = nullptr;
    int *color_slots = nullptr;  // slots of the (bx + by) even blocks, then the odd ones (the pair splat's two launches)
    int n_blocks = 0, n_color0 = 0, n_list = 0;
    std::vector<int32_t> list_key;
    bool have_list = false;
    void release() {
        for (int *p : {pixel_list, pixel_map, block_ids, block_slot, color_slots}) (void)hipFree(p);
        *this = PixelList{};
    }
};

// The adaptive sampler's state (nh_adaptive_api.hip): the blocks' sampler clones live from the outer sample 0 of a
// render to the end of the ranges that continue it, as the reference's samplers vector does
struct AdaptiveState {
    int n_blocks = 0, nbx = 0, nby = 0;
    int next_sample = -1;  // the outer sample a continuing nh_render must start at (-1: only 0 will do)
    int4 *blocks = nullptr;
    int *block_rank = nullptr, *active_list = nullptr, *next = nullptr;
    AdBlock *state = nullptr;
    unsigned *counts = nullptr, *h_count = nullptr;  // per-pass active counts; pinned copy of the one just decided
    int2 *pos = nullptr;
    float4 *rad = nullptr, *staging = nullptr;
    float2 *jit = nullptr;
    size_t slot_cap = 0;  // staging slots (and next entries) allocated
    unsigned long long *stats = nullptr;
    std::vector<int4> h_blocks;  // by rank
};

// The photon mapper's map (nh_photon_api.hip): lives from nh_photon_map_build to the next build or upload
struct PhotonState {
    bool built = false;
    std::vector<void *> bufs;      // everything the map owns on the device
    const float *tables = nullptr; // PhotonData's decode tables (nh_photon.h), uploaded on first use; not in bufs
    std::vector<float> h_tables;
    // deposit order (nh_get_photons)
    float *pos = nullptr;
    uint2 *bytes = nullptr;
    uint32_t *path = nullptr;
    int *bounce = nullptr;
    nh_photon_stats stats{};
};

struct nh_ctx {
    uint64_t id = 0;  // unique per context (process lifetime): identifies comm-set members
    std::shared_ptr<CommSet> comms;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // host copies needed to build primitive records
    std::vector<nh_shape> shapes;
    std::vector<float> V;
    std::vector<uint32_t> F;
    int width = 0, height = 0, border = 0, n_emitters = 0, integrator = 0;
    nh_filter filter{};
    nhd::DScene S{};
    nhd::DScene *d_scene = nullptr;  // device copy of S read by the kernels
    nhd::Traversal tv{};
    std::vector<void *> scene_bufs, bvh_bufs;
    bool has_scene = false, has_bvh = false;
    int depth = 0;
    int depth_wide = 0;  // stack bound of the wide traversal
    int wide_w = 4;      // children per wide node of tv.wnodes: 4, or 8 (NH_WIDE8=1)
    int n_node_f4 = 0, n_leaves = 0, n_prim_f4 = 0;  // GPU BVH sizes (float4 / int2 entries)
    std::vector<uint32_t> bvh_indices, shape_offset;
    // material key of each shape in the sorted queues (the two kPrimMatShift bits of its primitive records): its BSDF
    // type, or for a Disney BSDF a key no other BSDF type of the scene uses (nh_upload_scene)
    std::vector<int> shape_bsdf_type;
    std::vector<int> shape_bsdf_real;  // NH_BSDF_* of each shape
    int n_bsdf_types = 0;              // distinct BSDF types in the scene
    bool disney = false;               // a Disney BSDF, or a spot / directional light: the scene renders with the
                                       // nh_disney:: kernels (NH_LAUNCH)
    bool specular = false;             // a mirror or dielectric BSDF: long discrete chains, long chunk tails
    bool textured = false;             // a BSDF with an albedo texture
    bool normal_mapped = false;        // a shape with a normal map (the full bounce / tail bodies' NMAP instantiation)
    // path_mis, every BSDF diffuse with a constant albedo, every light an area light on a mesh with an emit_faces
    // record, no envmap, normal map or thin lens: the RR-ahead kernels' trait instantiations apply
    bool diffuse_area = false;
    // a shape without a BSDF / a non-vacuum medium: only the volumetric integrators render the scene (nh_render)
    bool bsdfless = false, has_media = false;
    int sampler = 0, adaptive_initial_uniform = 0;  // NH_SAMPLER_*; an adaptive scene renders through render_adaptive
    AdaptiveState ad;
    PhotonState photon;
    bool av_set = false;  // nh_set_av_params since the scene's upload (S.av_length)
    // chunk buffers of the av integrator's split pipeline (nh_pipeline.hip av_reserve): arrays of av_cap paths
    AvLaunch av{};
    std::vector<void *> av_bufs;
    size_t av_cap = 0;
    int2 *av_spill = nullptr;  // the wide traversal's per-ray spill area, av_spill_depth entries per path
    int av_spill_depth = 0;
    // host copies of the scene tables and the emit_faces count, for the LDS image of a small scene (build_small_image)
    std::vector<nhd::DShape> h_shapes;
    std::vector<nhd::DBsdf> h_bsdfs;
    std::vector<nhd::DEmitter> h_emitters;
    std::vector<float> h_area_cdf;
    int n_emit_faces = 0;
    // the LDS image of a small scene (WfLaunch::small_image; owned by bvh_bufs) and its table regions' float4 counts
    // (all 0: tables not staged)
    float4 *small_image = nullptr;
    int small_tab[5] = {0, 0, 0, 0, 0};
    // pair_kinds: small_image's pair records are arranged by kind (host/gpu_layout.cpp pair_layout; NH_PAIR_KINDS=0 at
    // the BVH's upload: the reference arrangement). The counting kernels' any-hit primitive counts depend on the test
    // order, so a collect_stats render stages small_image_ref, the same image in the reference arrangement (null
    // without pair_kinds: small_image is that image).
    bool pair_kinds = false;
    float4 *small_image_ref = nullptr;
    // the flat image of a scene whose tree is one leaf or a root with two leaves (host/gpu_layout.cpp flat_image, read
    // by trace_flat of the non-counting RR-ahead bounce kernels; owned by bvh_bufs); null: not flat, or NH_FLAT_TRACE=0
    const float4 *flat_image = nullptr;
    // records in the flat image's any-hit section (host/shadow_masks.cpp shadow_any_word: what the light samples'
    // any-hit queries test instead of every record); 0: the image has no such section (NH_ANY_LIST=0, nothing left out)
    int flat_any_records = 0;
    // Candidate masks of the camera rays' first closest hit (WfLaunch::pmask, host/primary_masks.cpp): built by
    // nh_render (ensure_primary_masks) from the uploaded camera, the primitive records (kept here when there are at
    // most 64) and the pixel list's blocks; every upload and every new pixel list frees them (drop_primary_masks), so
    // pmask is null or the table of the current scene and list. It stays null when the feature is absent.
    nh_camera camera{};
    std::vector<float> h_prims;  // 12 floats per record, as uploaded; empty: more than 64 records
    unsigned long long *pmask = nullptr;
    bool pmask_known = false;
    // Candidate masks of bounce 0's light samples (WfLaunch::smask; host/shadow_masks.cpp), built and freed with pmask.
    // h_emit_tris: the emitter faces' vertices, 9 floats each, when every emitter is an area light on a mesh without
    // vertex normals (else empty: no table). smask is null without a pmask table.
    std::vector<float> h_emit_tris;
    unsigned long long *smask = nullptr;
    float *fb = nullptr;
    size_t fb_floats = 0;
    float *rec = nullptr;  // (r, g, b) per sample
    size_t rec_cap = 0;  // entries
    int *block_rank = nullptr;
    int nbx = 0, nby = 0;
    PixelList px;
    float4 *staging = nullptr;
    size_t staging_cap = 0;  // float4 entries
    unsigned long long *counters = nullptr;  // [0-3] queries, nodes, boxes, prims; [4] invalid; [8-11] wavefront shadow share
    nh_render_stats stats{};
    // wavefront pipeline (nh_pipeline.hip): path pools, each on its own stream, and
    // the queue of chunks not yet started
    WfPool pools[kPools + kTails];  // [0, kPools): path pools; then the tail slots
    std::deque<WfJob> jobs;
    uint64_t job_seq = 0, splat_seq = 0;  // chunks are splatted into fb in submission order
    hipEvent_t fb_ev = nullptr;           // the last enqueued write of fb (clear or splat)
    bool fb_ev_set = false;
    uint64_t stats_comm_inits = 0;  // communicator cliques this context created as reduce root
};

// Frees the context's candidate-mask table. The caller has drained the pipeline (no chunk in flight reads it).
inline void drop_primary_masks(nh_ctx *c) {
    (void)hipFree(c->pmask);
    (void)hipFree(c->smask);
    c->pmask = nullptr;
    c->smask = nullptr;
    c->pmask_known = false;
}

// A launcher of a kernel that shades, from the set nh_upload_scene chose for the context's scene (nh_internal.h)
#define NH_LAUNCH(c, fn) ((c)->disney ? nh_disney::nh::fn : nh::fn)

// nh_pipeline.hip
void pool_free(WfPool &p);
int pipeline_drain(nh_ctx *c);  // runs every submitted chunk to completion
int check_device(nh_ctx *c, const char *where);
// nh_adaptive_api.hip: nh_render of a scene with the adaptive sampler (the request already validated as far as
// every scene's is, the pipeline drained); release of its buffers (nh_destroy, and every scene upload)
int render_adaptive(nh_ctx *c, const nh_render_req *q);
void adaptive_release(nh_ctx *c);
// nh_photon_api.hip: drops the context's photon map (every scene / BVH upload; nh_destroy also frees the tables)
void photon_release(nh_ctx *c, bool tables = false);
// nh_upload.hip: the DDisney side record of a Disney BSDF (nh_bsdf_query builds one too)
nhd::DDisney disney_record(const nh_bsdf &b);
void disney_set_record(nhd::DBsdf &o, const nhd::DDisney *rec);
int disney_upload(nh_ctx *c, std::vector<void *> &owner, const std::vector<nhd::DDisney> &recs,
                  const std::vector<float> &albedo, nhd::DDisney **out);

// nh_api.hip: the device record of one nh_bsdf outside a scene, for nh_bsdf_query and nh_ttest_bsdf. alb: `albedo`, or
// the BSDF's own when null; a Disney BSDF's side record is uploaded into `owner`
int query_bsdf_record(nh_ctx *c, std::vector<void *> &owner, const nh_bsdf *b, const float *albedo, nhd::DBsdf &o,
                      float alb[3]);

inline bool fail(nh_ctx *c, const std::string &m) {
    if (c) c->err = m;
    return false;
}

#define HIP_TRY(ctx, expr)                                                                               \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                              \
            return NH_ERR_DEVICE;                                                                        \
        }                                                                                                \
    } while (0)

template <typename T>
int upload(nh_ctx *c, std::vector<void *> &owner, const T *src, size_t n, const T **dst) {
    void *p = nullptr;
    // a multiple of 16 B: the LDS staging of small scenes copies whole float4s of every record array
    size_t bytes = (std::max<size_t>(n * sizeof(T), 16) + 15) / 16 * 16;
    HIP_TRY(c, hipMalloc(&p, bytes));
    owner.push_back(p);
    if (n) HIP_TRY(c, hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *dst = reinterpret_cast<const T *>(p);
    return NH_OK;
}

inline void free_all(std::vector<void *> &v) {
    for (void *p : v) (void)hipFree(p);
    v.clear();
}

