// A first measurement of the warp test (profiles/warp_rate.txt): per warp type the wall time of nh_warp_run at the
// reference's own table (host clock around the call, which creates its context and ends in a device synchronise), and
// the rate of warp_histogram_kernel alone from HIP events around one launch of that table's point count.
//   tools/bin/warp_rate [device]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nh_internal.h"

#define CHECK(expr)                                                                   \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) {                                                       \
            std::fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));           \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

static const char *const kNames[] = {"none", "disk", "sphere", "spherevol", "spherecap", "hemisphere", "cosinehemisphere",
                                     "beckmann", "henyeygreenstein", "schlick", "microfacet", "isophase", "anisophase"};

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char **argv) {
    const int device = argc > 1 ? std::atoi(argv[1]) : 0;
    CHECK(hipSetDevice(device));
    hipStream_t st;
    CHECK(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::printf("type | cells | points | nh_warp_run wall ms (median of 5 after 2) | histogram kernel ms (median of 20 "
                "after 3, HIP events) | Mpoints/s\n");
    for (int type = NH_WARP_NONE; type <= NH_WARP_ANISO_PHASE; ++type) {
        if (type == NH_WARP_SCHLICK) continue;
        const float slider = type == NH_WARP_HENYEY_GREENSTEIN ? 0.65f : (type == NH_WARP_ANISO_PHASE ? 0.35f : 0.5f);
        const float angle = type == NH_WARP_MICROFACET_BRDF ? 0.7f : 0.5f;
        std::vector<double> wall;
        nh_chi2_result r;
        for (int i = 0; i < 7; ++i) {
            const auto t0 = std::chrono::steady_clock::now();
            if (nh_warp_run(device, type, slider, angle, NH_LENS_DRAWS_RTL, 0, 0, 0, &r, nullptr)) {
                std::fprintf(stderr, "nh_warp_run: %s\n", nh_host_last_error());
                return 1;
            }
            const auto t1 = std::chrono::steady_clock::now();
            if (i >= 2) wall.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        }
        WarpHist h;
        std::memset(&h, 0, sizeof(h));
        h.w.type = type;
        nh_warp_map_parameter(type, slider, &h.w.parameter);
        nh_warp_wi(angle, h.w.wi);
        h.w.bsdf.type = NH_BSDF_MICROFACET;
        h.w.bsdf.alpha = h.w.parameter;
        h.w.bsdf.int_ior = 1.5046f;
        h.w.bsdf.ext_ior = 1.000277f;
        h.w.bsdf.ks = 1.f;
        h.yres = 51;
        h.xres = (type == NH_WARP_NONE || type == NH_WARP_DISK) ? 51 : 102;
        const int cells = h.xres * h.yres;
        h.n = 1000 * cells;
        const int64_t max_lanes = (int64_t)kChi2MaxGroups * kChi2Block;
        h.run = (int)std::max<int64_t>(kChi2MinRun, ((int64_t)h.n + max_lanes - 1) / max_lanes);
        h.rtl = 1;
        h.sub_tables = cells * (kChi2Block / 64) <= NH_CHI2_MAX_CELLS ? 1 : 0;
        uint32_t *counts = nullptr;
        CHECK(hipMalloc(&counts, ((size_t)cells + 1) * sizeof(uint32_t)));
        CHECK(hipMemsetAsync(counts, 0, ((size_t)cells + 1) * sizeof(uint32_t), st));
        h.counts = counts;
        h.nan_points = counts + cells;
        std::vector<double> ms;
        for (int i = 0; i < 23; ++i) {
            CHECK(hipEventRecord(e0, st));
            nh_disney::nh::launch_warp_histogram(h, st);
            CHECK(hipEventRecord(e1, st));
            CHECK(hipEventSynchronize(e1));
            float t = 0.f;
            CHECK(hipEventElapsedTime(&t, e0, e1));
            if (i >= 3) ms.push_back(t);
        }
        CHECK(hipGetLastError());
        CHECK(hipFree(counts));
        const double k = median(ms);
        std::printf("%s | %dx%d | %d | %.2f | %.4f | %.0f\n", kNames[type], h.yres, h.xres, h.n, median(wall), k,
                    h.n / k / 1e3);
    }
    return 0;
}
