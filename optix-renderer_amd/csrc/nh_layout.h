// GPU BVH / lens-table layout constants shared by the kernels (nh_traverse.h, nh_device.h) and the host code that
// builds those arrays (host/gpu_layout.cpp). Plain C++: no HIP header, so the host library compiles it too.
#pragma once

namespace nhd {

// lens-stream tables (DScene::lens_lo / lens_hi): rounds 256 h + l, h < kLensHi
constexpr int kLensLo = 256, kLensHi = 65536;

// primitive record type / leaf-end bits (word 2 .w of the record), and the BSDF type of the owning
// shape in bits 2-3 (the material key of the sorted shade queues)
constexpr int kPrimSphere = 1, kPrimLeafEnd = 2, kPrimMatShift = 2;
// an isolated sphere (record 2 .w bit; record 1 .x holds the host's margin m): see nh_traverse.h trace_next
constexpr int kPrimIsolated = 16;

// float4s of one 4-wide node (nh_traverse.h Tracer4: 128 B, one cache line); an 8-wide node is two of them
constexpr int kWideF4 = 8;
// child ref of an unused wide-node slot
constexpr int kWideEmpty = (int)0x80000000;

// The flat image of a scene whose tree is one leaf, or a root with two leaves (host/gpu_layout.cpp flat_image,
// nh_traverse.h trace_flat), in float4s:
//   [0] root min xyz, int bits: kFlatLeftEq / kFlatRightEq -- that child's box is bit-equal to the root's;
//       kFlatAnyList -- the image has an any-hit section
//   [1] root max xyz, int leaves (1 or 2)
//   [2] left min xyz, int left leaf's triangle pairs | sphere pairs << 16     [3] left max xyz, its any-hit counts
//   [4] right min xyz, int right leaf's counts (0 with one leaf)              [5] right max xyz, its any-hit counts
//   [6..] the pair records (kPairF4 float4 each), the left leaf's triangle pairs, its sphere pairs, then the right leaf's
//   [kFlatAnyOff..] with kFlatAnyList: the any-hit section -- pair records of the same form over the records the
//       scene-wide any-hit word keeps (host/shadow_masks.cpp), each leaf's paired among themselves, in the same order;
//       the any-hit counts are 0 without it. Between the closest-hit records and the section: zeros.
// A single leaf is the left one with the root's box.
constexpr int kPairF4 = 6;  // float4s of a pair record (nh_traverse.h Traversal::ppairs)
constexpr int kFlatHeaderF4 = 6, kFlatMaxPairs = 16;
constexpr int kFlatLeftEq = 1, kFlatRightEq = 2, kFlatAnyList = 4;
constexpr int kFlatAnyOff = kFlatHeaderF4 + kPairF4 * kFlatMaxPairs;

// deepest per-lane LDS stack of the binary-tree kernels (DEPTH template)
constexpr int kMaxStack = 128;

}  // namespace nhd
