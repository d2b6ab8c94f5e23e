// Host-side layout of what the traversal and camera kernels read: the GPU BVH (binary nodes, leaf table, primitive
// records, wide collapse), the isolated-sphere marks, the block spiral, the lens-stream tables and the nee_finite
// scene flag. Plain C++ (no HIP): part of both libraries, and checked on the CPU by tests/c/gpu_layout_check.cpp.
// The record formats are described where the kernels read them (csrc/nh_traverse.h); the constants both sides share
// are in csrc/nh_layout.h.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "nori_hip.h"

namespace nh {

// stand-ins for HIP's float4 / int2 / ulonglong2: the C-ABI layer uploads these arrays as they are
struct f4 {
    float x, y, z, w;
};
struct i2 {
    int x, y;
};
struct u64x2 {
    uint64_t x, y;
};

struct GpuBvh {
    std::vector<f4> nodes;   // 4 per inner node, left-first DFS order
    std::vector<i2> leaves;  // (start, count) into the primitive records
    std::vector<f4> prims;   // 3 per primitive in leaf order, leaf-end bits set, plus one zero record past the end
    std::vector<f4> wide;    // wide_w / 4 * kWideF4 per wide node, the top n_top numbered first
    std::vector<uint32_t> shape_offset;  // first primitive id of each shape, and the total
    int root_kind = 0;       // 0 empty, 1 inner root, 2 the root is a leaf
    float root_min[3] = {0.f, 0.f, 0.f}, root_max[3] = {0.f, 0.f, 0.f};
    uint32_t tree_depth = 0;  // deepest level of the binary tree (root = 0), measured
    int depth_wide = 1;       // stack bound of the wide traversal: (wide_w - 1) deferred entries per wide level, + 1
    int n_top = 0;
    int iso_spheres = 0;
};

// The GPU BVH of `b` over the scene's shapes (V, F: the scene's vertex and face arrays; shape_mat_key: the
// kPrimMatShift bits of each shape's records; shape_bsdf_real: its NH_BSDF_*). wide_w: 4 or 8 children per wide node;
// top_k: wide nodes to number first. NH_OK, or an error code with its message in err.
int build_gpu_bvh(const nh_bvh_desc &b, const std::vector<nh_shape> &shapes, const std::vector<float> &V,
                  const std::vector<uint32_t> &F, const std::vector<int> &shape_mat_key,
                  const std::vector<int> &shape_bsdf_real, int wide_w, int top_k, GpuBvh &out, std::string &err);

// the two steps of the wide tree, as build_gpu_bvh runs them
std::vector<f4> collapse_wide(const std::vector<f4> &nodes, const std::vector<i2> &leaves, int &depth_out, int W = 4);
int number_top_first(std::vector<f4> &wide, const float root_min[3], const float root_max[3], int K, int W = 4);

std::vector<int> spiral_rank(int w, int h, int bs, int &nbx, int &nby);
std::vector<uint32_t> serial_ray_index(int w, int h, int bs);

struct LensTables {
    std::vector<u64x2> pix, lo;
    std::vector<uint64_t> hi;
};
LensTables lens_tables(int w, int h);

bool nee_finite(const nh_scene_desc *d);

// Per-block candidate masks of the camera rays' first closest hit (primary_masks.cpp). prims: the n_records primitive
// records as the device reads them (3 f4 each, record index k); blocks: ids (by * nbx + bx) of the rendered 32x32
// blocks. masks[i] bit k: record k can be hit by a camera ray of block blocks[i]. False, and no table, when the scene
// has more than 64 records or the camera a lens (or its transform cannot be inverted).
bool primary_masks(const nh_camera &cam, const f4 *prims, int n_records, const int32_t *blocks, int n_blocks,
                   std::vector<uint64_t> &masks);
// the pad in pixels a block's rectangle is grown by: at least 2, a 256th of the larger image side
int primary_mask_pad(int width, int height);
// in_front[k]: every point of record k passes the masks' in-front-of-camera condition (else the record is a candidate
// of every block). False when primary_masks would build no table.
bool primary_mask_in_front(const nh_camera &cam, const f4 *prims, int n_records, std::vector<char> &in_front);

// Candidate masks of the light sample's any-hit query (shadow_masks.cpp). emit_faces: the vertices of every emitter
// face, 9 floats each -- n_faces > 0 only when every emitter of the scene is an area light on a mesh without vertex
// normals (the caller's part), else 0: nothing is left out.
// The emitter-side word: bit k clear when no shadow ray of any bounce can be accepted by record k (all ones with more
// than 64 records).
uint64_t shadow_emitter_mask(const f4 *prims, int n_records, const float *emit_faces, int n_faces);
// The scene-wide any-hit word: the emitter-side word less the supporting walls -- triangle records that have every
// emitter vertex well in front of their plane and every possible far end of a shadow ray (a float hit point on any
// record, of a ray from the camera or from another such point) on that same closed side, so that the ray ends, kEps
// short of the far end, before their float test can accept it. Bit k set: record k stays. All ones where
// shadow_emitter_mask is.
uint64_t shadow_any_word(const nh_camera &cam, const f4 *prims, int n_records, const float *emit_faces, int n_faces);
// NH_ANY_LIST=0 (read at every call; the BVH upload calls it once): the flat image gets no any-hit section
bool any_list_knob();
// The emit_faces of a scene: every emitting face's vertices when every emitter is an area light on a mesh without vertex
// normals; empty otherwise (a point, spot, directional or envmap light, a sphere light, a mesh light with normals).
std::vector<float> shadow_emitter_faces(const nh_scene_desc &d);
// The per-block words of bounce 0 (indexing and absence as primary_masks): masks[i] bit k clear when no shadow ray
// that ends at a first hit of block blocks[i]'s camera rays can be accepted by record k. Each holds the emitter-side
// word's zeros too.
bool shadow_block_masks(const nh_camera &cam, const f4 *prims, int n_records, const float *emit_faces, int n_faces,
                        const int32_t *blocks, int n_blocks, std::vector<uint64_t> &masks);

// Which records share a pair record of a small scene's LDS image (csrc/nh_traverse.h leaf_test<.., PAIRS>). There are
// as many pair positions as records; a leaf's pairs start at the position of its first record.
//   slots[p]  = (slot 0 record, slot 1 record or -1: slot 0 has no partner); (-1, -1): position p is not used
//   leaves[l] = (first pair position, triangle pairs | sphere pairs << 16)
// by_kind: each leaf's triangles in record order two by two, then its spheres two by two -- no pair mixes kinds, and a
// leaf has at most one single triangle and one single sphere (the last of its kind). Otherwise the reference
// arrangement: position p = records (p, p + 1) for every p, and leaves[l].y = 0, which sends leaf_test to its loop over
// the leaf's records in order. prims: the n_records primitive records (3 f4 each); the leaves' ranges lie inside
// [0, n_records) and do not overlap.
struct PairLayout {
    std::vector<i2> slots, leaves;
};
PairLayout pair_layout(const i2 *leaves, int n_leaves, const f4 *prims, int n_records, bool by_kind);

// The flat image of a scene the fused bounce kernels traverse without a tree walk (csrc/nh_traverse.h trace_flat; the
// format: csrc/nh_layout.h kFlatHeaderF4). A scene is flat when `allowed` (the caller's part: the scene is staged
// small, its pair records are arranged by kind, and flat_trace_knob()), its tree is one leaf (n_leaves 1) or a root
// whose two children are both leaves (n_leaves 2: leaf 0 the left child, leaf 1 the right one), and pl -- the
// arrangement by kind of those leaves -- has at most kFlatMaxPairs pair positions in use.
//   boxes: 18 floats -- the root's box (min xyz, max xyz), the left child's, the right child's (one leaf: the last two
//          are not read)
//   data:  the image (empty when not flat); its pair records hold what the device computes for the LDS image's: p0, the
//          edges p1 - p0 and p2 - p0 by the same IEEE subtractions, the flag words and the record indices
//   box_equal: kFlatLeftEq / kFlatRightEq bits -- the child's six bounds have the bit patterns of the root's
//   any_word: the scene-wide any-hit word (shadow_any_word; bit k set: record k stays). Unless it is all ones over the
//          records, the image gets an any-hit section (any_list): at kFlatHeaderF4 + kPairF4 * kFlatMaxPairs, each
//          leaf's kept records paired again by pair_layout's rules, the left leaf's first; header words [3].w / [5].w
//          hold each leaf's counts (triangle pairs | sphere pairs << 16) and [0].w the kFlatAnyList bit. box_equal
//          does not hold that bit.
struct FlatImage {
    bool flat = false;
    bool any_list = false;
    int box_equal = 0;
    std::vector<f4> data;
};
FlatImage flat_image(const float boxes[18], const i2 *leaves, int n_leaves, const f4 *prims, int n_records,
                     const PairLayout &pl, bool allowed, uint64_t any_word = ~(uint64_t)0);
// NH_FLAT_TRACE=0 (read at every call; the BVH upload calls it once) turns flat traversal off
bool flat_trace_knob();

}  // namespace nh
