// Per-block candidate masks for the camera rays' first closest hit ("Primary candidate masks").
//
// A pinhole camera ray through raster position (x, y) can only be accepted by a primitive whose projection holds
// (x, y). For each rendered 32x32 block this file lists, as one bit per primitive record, the records whose projected
// bounding box comes within a pad of the block's pixel rectangle; bounce 0 of the fused bounce kernels skips the pair
// records none of whose bits is set (csrc/nh_traverse.h leaf_test<.., MASKED>). Leaving out a record that could not
// have accepted the ray changes neither the closest hit nor the maxt the other tests see, so the masks only have to be
// conservative. Everything here is double precision on the float inputs the kernels read.
//
// Plain C++ (no HIP): part of both libraries; checked on the CPU by tests/test_primary_masks_host.py.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "gpu_layout.h"
#include "nh_host.h"

#include "../csrc/nh_layout.h"

namespace nh {

namespace {

struct V3 {
    double x, y, z;
};

// inverse of a row-major 4x4 by Gauss-Jordan with partial pivoting; false when singular
bool invert4(const float *m, double inv[16]) {
    double a[4][8];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            a[r][c] = m[4 * r + c];
            a[r][4 + c] = r == c ? 1.0 : 0.0;
        }
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        for (int r = c + 1; r < 4; ++r)
            if (std::fabs(a[r][c]) > std::fabs(a[piv][c])) piv = r;
        if (!(std::fabs(a[piv][c]) > 0.0) || !std::isfinite(a[piv][c])) return false;
        for (int k = 0; k < 8; ++k) std::swap(a[c][k], a[piv][k]);
        const double s = 1.0 / a[c][c];
        for (int k = 0; k < 8; ++k) a[c][k] *= s;
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double f = a[r][c];
            for (int k = 0; k < 8; ++k) a[r][k] -= f * a[c][k];
        }
    }
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) inv[4 * r + c] = a[r][4 + c];
    return true;
}

struct Projector {
    double w2c[16];
    double m[16];  // sample_to_camera
    double width, height;

    // The raster position whose camera ray (csrc/nh_shade.h camera_ray: the direction of sample_to_camera * (sx, sy, 0,
    // 1) after its homogeneous division, from the camera-space origin) passes through world point p. False unless p
    // lies in front of the camera by a clear margin (camera space z above 1e-3 of its distance) and the position is
    // finite: the caller then keeps the record for every block.
    bool raster(const V3 &p, double &rx, double &ry) const {
        double c[4];
        for (int r = 0; r < 4; ++r) c[r] = w2c[4 * r] * p.x + w2c[4 * r + 1] * p.y + w2c[4 * r + 2] * p.z + w2c[4 * r + 3];
        if (!(std::fabs(c[3]) > 0.0)) return false;
        const V3 q{c[0] / c[3], c[1] / c[3], c[2] / c[3]};
        const double dist = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
        if (!std::isfinite(dist) || !(q.z > 1e-3 * dist) || !(dist > 0.0)) return false;
        // m[:3, 0] sx + m[:3, 1] sy - lambda q = -m[:3, 3]  (the ray's direction is parallel to q), by Cramer's rule
        const double a0[3] = {m[0], m[4], m[8]}, a1[3] = {m[1], m[5], m[9]}, a2[3] = {-q.x, -q.y, -q.z};
        const double b[3] = {-m[3], -m[7], -m[11]};
        const auto det3 = [](const double *u, const double *v, const double *w) {
            return u[0] * (v[1] * w[2] - v[2] * w[1]) - v[0] * (u[1] * w[2] - u[2] * w[1]) +
                   w[0] * (u[1] * v[2] - u[2] * v[1]);
        };
        const double det = det3(a0, a1, a2);
        if (!(std::fabs(det) > 0.0)) return false;
        const double sx = det3(b, a1, a2) / det, sy = det3(a0, b, a2) / det, lambda = det3(a0, a1, b) / det;
        const double hw = m[12] * sx + m[13] * sy + m[15];
        // the same sense, not the opposite one: direction = (lambda / hw) q
        if (!std::isfinite(sx) || !std::isfinite(sy) || !(lambda / hw > 0.0)) return false;
        rx = sx * width;
        ry = sy * height;
        return true;
    }
};

}  // namespace

int primary_mask_pad(int width, int height) { return std::max(2, (std::max(width, height) + 255) / 256); }

namespace {

// the raster bounding box of a record; everywhere: a candidate for every block (one of its points fails
// Projector::raster's in-front-of-camera condition)
struct Box {
    bool everywhere;
    double x0, y0, x1, y1;
};

// every record's raster box; false when the feature is absent (more than 64 records, a lens, a singular transform)
bool record_boxes(const nh_camera &cam, const f4 *prims, int n_records, std::vector<Box> &box) {
    if (n_records < 0 || n_records > 64 || cam.lens_radius > 1e-4f || cam.width <= 0 || cam.height <= 0) return false;
    Projector pr;
    if (!invert4(cam.camera_to_world, pr.w2c)) return false;
    for (int i = 0; i < 16; ++i) pr.m[i] = cam.sample_to_camera[i];
    pr.width = cam.width;
    pr.height = cam.height;
    // the camera's world-space origin, as camera_ray forms it
    const float *cw = cam.camera_to_world;
    const V3 org{(double)cw[3] / cw[15], (double)cw[7] / cw[15], (double)cw[11] / cw[15]};

    box.assign((size_t)n_records, Box{});
    for (int k = 0; k < n_records; ++k) {
        const f4 a = prims[3 * k], b = prims[3 * k + 1], c = prims[3 * k + 2];
        int bits;
        std::memcpy(&bits, &c.w, sizeof(bits));
        V3 pts[8];
        int n_pts;
        if (bits & nhd::kPrimSphere) {
            // the corners of the sphere's box, grown by more than what sphere_test's float discriminant can be off by
            // near the silhouette: rounding of about 2^-24 (2 D)^2 in a value whose zero lies where the squared impact
            // parameter equals r^2, that is about 2^-23 D^2 / r in the impact parameter itself, D = the farthest
            // distance of the sphere from the camera. 64 times that, plus a thousandth of the radius.
            const double r = std::fabs((double)a.w);
            const double dx = a.x - org.x, dy = a.y - org.y, dz = a.z - org.z;
            const double far_d = std::sqrt(dx * dx + dy * dy + dz * dz) + r;
            const double g = r + 1e-3 * r + 64.0 * std::ldexp(1.0, -24) * far_d * far_d / std::max(r, 1e-300);
            n_pts = 8;
            for (int i = 0; i < 8; ++i)
                pts[i] = V3{a.x + (i & 1 ? g : -g), a.y + (i & 2 ? g : -g), a.z + (i & 4 ? g : -g)};
        } else {
            n_pts = 3;
            pts[0] = V3{a.x, a.y, a.z};
            pts[1] = V3{b.x, b.y, b.z};
            pts[2] = V3{c.x, c.y, c.z};
        }
        Box bx{false, INFINITY, INFINITY, -INFINITY, -INFINITY};
        for (int i = 0; i < n_pts && !bx.everywhere; ++i) {
            double rx, ry;
            if (!pr.raster(pts[i], rx, ry)) {
                bx.everywhere = true;
                break;
            }
            bx.x0 = std::min(bx.x0, rx);
            bx.x1 = std::max(bx.x1, rx);
            bx.y0 = std::min(bx.y0, ry);
            bx.y1 = std::max(bx.y1, ry);
        }
        box[(size_t)k] = bx;
    }
    return true;
}

}  // namespace

bool primary_mask_in_front(const nh_camera &cam, const f4 *prims, int n_records, std::vector<char> &in_front) {
    std::vector<Box> box;
    in_front.clear();
    if (!record_boxes(cam, prims, n_records, box)) return false;
    for (const Box &b : box) in_front.push_back(b.everywhere ? 0 : 1);
    return true;
}

bool primary_masks(const nh_camera &cam, const f4 *prims, int n_records, const int32_t *blocks, int n_blocks,
                   std::vector<uint64_t> &masks) {
    masks.clear();
    std::vector<Box> box;
    if (!record_boxes(cam, prims, n_records, box)) return false;

    const double pad = primary_mask_pad(cam.width, cam.height);
    const int nbx = (cam.width + 31) / 32, nby = (cam.height + 31) / 32;
    masks.assign((size_t)std::max(n_blocks, 0), 0);
    for (int i = 0; i < n_blocks; ++i) {
        const int bid = blocks[i];
        if (bid < 0 || bid >= nbx * nby) {  // not a block of this image: nothing culled
            masks[(size_t)i] = ~(uint64_t)0;
            continue;
        }
        const int bx = bid % nbx, by = bid / nbx;
        // raster positions of the block's samples: pixel + jitter, jitter in [0, 1)
        const double x0 = 32.0 * bx - pad, x1 = std::min(32.0 * bx + 32.0, (double)cam.width) + pad;
        const double y0 = 32.0 * by - pad, y1 = std::min(32.0 * by + 32.0, (double)cam.height) + pad;
        uint64_t mk = 0;
        for (int k = 0; k < n_records; ++k) {
            const Box &b = box[(size_t)k];
            const bool miss = !b.everywhere && (b.x1 < x0 || b.x0 > x1 || b.y1 < y0 || b.y0 > y1);
            if (!miss) mk |= (uint64_t)1 << k;
        }
        masks[(size_t)i] = mk;
    }
    return true;
}

}  // namespace nh

extern "C" {

int nh_primary_masks(const nh_camera *camera, const float *records, int32_t n_records, const int32_t *blocks,
                     int32_t n_blocks, uint64_t *masks, int32_t *built) {
    if (!camera || !built || n_records < 0 || n_blocks < 0 || (n_records > 0 && !records) ||
        (n_blocks > 0 && (!blocks || !masks))) {
        nh::set_host_error("nh_primary_masks: invalid argument");
        return NH_ERR_INVALID;
    }
    static_assert(sizeof(nh::f4) == 4 * sizeof(float), "records are read as float4 triples");
    std::vector<uint64_t> m;
    *built = nh::primary_masks(*camera, reinterpret_cast<const nh::f4 *>(records), n_records, blocks, n_blocks, m) ? 1 : 0;
    if (*built && n_blocks > 0) std::memcpy(masks, m.data(), (size_t)n_blocks * sizeof(uint64_t));
    return NH_OK;
}

int32_t nh_primary_mask_pad(int32_t width, int32_t height) { return nh::primary_mask_pad(width, height); }

}  // extern "C"
