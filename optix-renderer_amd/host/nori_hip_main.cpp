// nori_hip: headless equivalent of the reference's `nori <scene.xml>` entry
// (src/utils/main.cpp:32-114 + RenderThread::renderThreadMain, render.cpp:232-419),
// rendering the scene's path_mis / path_mats integrator on one MI355X through the
// C-ABI, applying the scene's <denoiser> (render.cpp:368-369), and writing <scene>.exr next to the input
// (Bitmap::save, bitmap.cpp:82-110). A scene with the adaptive sampler also prints "Total Samples Placed" and writes
// <scene>_variance.exr (render.cpp:373, :392-413).
//
//   nori_hip scene.xml [--spp N] [--width W --height H] [--device D] [--ordered] [--pfm out.pfm] [--png] [--seed S]
// --png also writes <scene>.png as Bitmap::saveToLDR (bitmap.cpp:122-140; the reference's hdrToLdr). --seed: the base
// of the per-path streams (default 0).
// A file whose root is a <test type="ttest"> runs the reference's t-tests instead (StudentsTTest::execute,
// src/utils/ttest.cpp): per test the sample mean, variance, t-statistic and verdict, then "Passed p/t tests."; the
// exit status is 0 only if all passed. A <test type="chi2test"> root runs the reference's chi^2 tests
// (ChiSquareTest::execute, src/utils/chi2test.cpp) the same way.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nori_hip.h"

static int die(const char *what, const char *msg) {
    std::fprintf(stderr, "nori_hip: %s: %s\n", what, msg);
    return 1;
}

// StudentsTTest::execute's report (ttest.cpp:163-241, hypothesis.h:324-342) for a <test> file run on the HIP path
// (nh_test_run); 0 only if every test passed
static int run_tests(const std::string &path, const nh_test *test, int device, unsigned long long seed) {
    nh_test_desc td;
    nh_test_get_desc(test, &td);
    const size_t n_tests = td.n_bsdfs ? (size_t)td.n_bsdfs * td.n_references : td.n_scenes;
    std::vector<nh_test_result> res(n_tests ? n_tests : 1);
    int32_t n = 0;
    if (nh_test_run(device, path.c_str(), seed, res.data(), (int32_t)res.size(), &n)) return die("test", nh_host_last_error());
    const double level = 1.0 - std::pow(1.0 - (double)td.significance_level, 1.0 / (double)td.n_references);
    int passed = 0;
    for (int i = 0; i < n && i < (int)res.size(); ++i) {
        const nh_test_result &r = res[i];
        std::printf("------------------------------------------------------\n");
        if (td.n_bsdfs) std::printf("Testing (angle=%g): BSDF %d\nDrawing %d samples .. \n", r.angle, i / (int)td.n_references, r.sample_count);
        else std::printf("Testing scene: %d\nGenerating %d paths.. \n", i, r.sample_count);
        const double t = std::fabs(r.mean - r.reference) * std::sqrt(r.sample_count / std::max(r.variance, 1e-5));
        std::printf("Sample mean = %g (reference value = %g)\n", r.mean, r.reference);
        std::printf("Sample variance = %g\n", r.variance);
        std::printf("t-statistic = %g (d.o.f. = %d)\n", t, r.sample_count - 1);
        std::printf("%s the null hypothesis (p-value = %g, significance level = %g)\n\n",
                    r.accepted ? "Accepted" : "***** Rejected *****", r.p_value, level);
        passed += r.accepted ? 1 : 0;
    }
    std::printf("Passed %d/%d tests.\n", passed, (int)n);
    return passed == n ? 0 : 1;
}

// hypothesis::chi2_test's message (hypothesis.h:163-234) for one verdict; true when the null hypothesis was accepted
static bool report_chi2(const nh_chi2_result &r, double min_exp_frequency) {
    if (r.kind == NH_CHI2_REJECTED_ZERO_CELL) {
        std::printf("Encountered %g samples in a cell with expected frequency 0. Rejecting the null hypothesis!\n\n",
                    r.statistic);
        return false;
    }
    if (r.pooled_cells > 0)
        std::printf("Pooled %d to ensure sufficiently high expected cell frequencies (>%g)\n", r.pooled_cells,
                    min_exp_frequency);
    if (r.kind == NH_CHI2_REJECTED_DOF) {
        std::printf("The number of degrees of freedom (%d) is too low!\n\n", r.dof);
        return false;
    }
    std::printf("Chi^2 statistic = %g (d.o.f. = %d)\n", r.statistic, r.dof);
    std::printf("%s the null hypothesis (p-value = %g, significance level = %g)\n\n",
                r.accepted ? "Accepted" : "***** Rejected *****", r.p_value, r.level);
    return r.accepted != 0;
}

// ChiSquareTest::execute's report (chi2test.cpp:147-233, hypothesis.h:163-234) for a <test type="chi2test"> file run
// on the HIP path (nh_chi2_run); 0 only if every test passed. The chi2test_%i.m dumps are not written.
static int run_chi2_tests(const std::string &path, const nh_test *test, int device) {
    nh_test_desc td;
    nh_chi2_params cp;
    nh_test_get_desc(test, &td);
    if (nh_test_get_chi2_params(test, &cp)) return die("test", nh_host_last_error());
    const size_t n_tests = (size_t)td.n_bsdfs * (size_t)(cp.test_count > 0 ? cp.test_count : 0);
    std::vector<nh_chi2_result> res(n_tests ? n_tests : 1);
    int32_t n = 0;
    if (nh_chi2_run(device, path.c_str(), res.data(), (int32_t)res.size(), &n)) return die("test", nh_host_last_error());
    int passed = 0;
    for (int i = 0; i < n && i < (int)res.size(); ++i) {
        const nh_chi2_result &r = res[i];
        std::printf("------------------------------------------------------\n");
        std::printf("Testing: BSDF %d (wi = [%g, %g, %g])\n", i / cp.test_count, r.wi[0], r.wi[1], r.wi[2]);
        std::printf("Accumulating %d samples into a %dx%d contingency table .. done.\n", r.sample_count, cp.resolution,
                    2 * cp.resolution);
        std::printf("Integrating expected frequencies .. done.\n");
        passed += report_chi2(r, (double)cp.min_exp_frequency) ? 1 : 0;
    }
    std::printf("Passed %d/%d tests.\n", passed, (int)n);
    return passed == n ? 0 : 1;
}

// WarpTest::runTest (warptest.cpp:439-562) on the HIP path (nh_warp_run), headless: the verdict text of
// hypothesis::chi2_test, which the GUI shows in its message box; 0 on accept, 1 on reject
static const char *const kWarpNames[] = {"none", "disk", "sphere", "spherevol", "spherecap", "hemisphere", "cosinehemisphere",
                                         "beckmann", "henyeygreenstein", "schlick", "microfacet", "isophase", "anisophase"};
static int run_warp_test(int argc, char **argv) {
    if (argc < 3) return die("--warptest", "needs a warp name");
    int type = -1, device = 0, xres = 0, yres = 0, samples = 0, order = NH_LENS_DRAWS_RTL;
    for (int t = 0; t < (int)(sizeof(kWarpNames) / sizeof(kWarpNames[0])); ++t)
        if (std::strcmp(argv[2], kWarpNames[t]) == 0) type = t;
    if (type < 0) return die("--warptest: unknown warp", argv[2]);
    float param = 0.5f, angle = 0.5f;
    for (int i = 3; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() { return i + 1 < argc ? argv[++i] : (char *)"0"; };
        if (a == "--param") param = (float)std::atof(next());
        else if (a == "--angle") angle = (float)std::atof(next());
        else if (a == "--res") {
            xres = std::atoi(next());
            yres = std::atoi(next());
        } else if (a == "--samples") samples = std::atoi(next());
        else if (a == "--ltr") order = NH_LENS_DRAWS_LTR;
        else if (a == "--device") device = std::atoi(next());
        else return die("argument", a.c_str());
    }
    if ((xres || yres) && !samples) samples = 1000 * xres * yres;  // runTest's own density
    nh_chi2_result r;
    if (nh_warp_run(device, type, param, angle, order, xres, yres, samples, &r, nullptr))
        return die("warptest", nh_host_last_error());
    float value = 0.f;
    nh_warp_map_parameter(type, param, &value);
    std::printf("Testing warp: %s (parameter = %g, wi = [%g, %g, %g])\n", kWarpNames[type], value, r.wi[0], r.wi[1], r.wi[2]);
    std::printf("Accumulated %d points .. done.\nIntegrating expected frequencies .. done.\n", r.sample_count);
    return report_chi2(r, 5.0) ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: nori_hip scene.xml [--spp N] [--width W --height H] [--device D] [--ordered] [--pfm out] [--png] [--seed S]\n"
                             "       nori_hip --warptest <name> [--param s] [--angle s] [--res X Y] [--samples N] [--ltr] [--device D]\n");
        return 1;
    }
    if (std::strcmp(argv[1], "--warptest") == 0) return run_warp_test(argc, argv);
    std::string scene_path = argv[1], pfm;
    bool png = false;
    int spp = 0, w = 0, h = 0, device = 0, traversal = NH_TRAVERSAL_REFERENCE;
    unsigned long long seed = 0;
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() { return i + 1 < argc ? argv[++i] : (char *)"0"; };
        if (a == "--spp") spp = std::atoi(next());
        else if (a == "--width") w = std::atoi(next());
        else if (a == "--height") h = std::atoi(next());
        else if (a == "--device") device = std::atoi(next());
        else if (a == "--ordered") traversal = NH_TRAVERSAL_ORDERED;
        else if (a == "--pfm") pfm = next();
        else if (a == "--png") png = true;
        else if (a == "--seed") seed = std::strtoull(next(), nullptr, 0);
        else return die("argument", a.c_str());
    }
    // a <test> root runs the reference's t-tests (StudentsTTest::execute) instead of a render
    nh_test *test = nullptr;
    const int trc = nh_test_load_xml(scene_path.c_str(), &test);
    if (trc == NH_OK) {
        nh_test_desc td;
        nh_test_get_desc(test, &td);
        const int rc = td.type == NH_TEST_CHI2TEST ? run_chi2_tests(scene_path, test, device)
                                                   : run_tests(scene_path, test, device, seed);
        nh_test_free(test);
        return rc;
    }
    if (trc != NH_ERR_INVALID) return die("load", nh_host_last_error());  // (NH_ERR_INVALID: not a <test> root)
    nh_scene *scene = nullptr;
    if (nh_scene_load_xml(scene_path.c_str(), &scene)) return die("load", nh_host_last_error());
    if (w > 0 && h > 0) nh_scene_set_resolution(scene, w, h);
    if (spp > 0) nh_scene_set_sample_count(scene, spp);
    nh_scene_desc desc;
    nh_scene_get_desc(scene, &desc);
    auto t0 = std::chrono::steady_clock::now();
    nh_bvh *bvh = nullptr;
    if (nh_bvh_build(&desc, 0, &bvh)) return die("bvh", nh_host_last_error());
    nh_bvh_desc bd;
    nh_bvh_get_desc(bvh, &bd);
    auto t1 = std::chrono::steady_clock::now();
    nh_ctx *ctx = nullptr;
    if (nh_create(device, &ctx)) return die("device", "cannot create a context on the requested GPU");
    if (nh_upload_scene(ctx, &desc) || nh_upload_bvh(ctx, &bd)) return die("upload", nh_last_error(ctx));
    if (desc.integrator == NH_INTEGRATOR_PHOTONMAPPER) {  // PhotonMapper::preprocess and its report (photonmapper.cpp:63, :152)
        nh_photon_params pp;
        nh_scene_get_photon_params(scene, &pp);
        std::printf("Gathering %d photons .. ", pp.photon_count);
        std::fflush(stdout);
        if (nh_photon_map_build(ctx, &pp, 0, 0)) return die("photon map", nh_last_error(ctx));
        nh_photon_stats ps;
        nh_get_photon_stats(ctx, &ps);
        std::printf("Emitted %d Photons.\n", ps.emitted);
    }
    if (desc.integrator == NH_INTEGRATOR_AV) {  // the occlusion ray's length travels beside the descriptor
        nh_av_params ap;
        nh_scene_get_av_params(scene, &ap);
        if (nh_set_av_params(ctx, &ap)) return die("av", nh_last_error(ctx));
    }
    nh_render_req req;
    std::memset(&req, 0, sizeof(req));
    req.sample_begin = 0;
    req.sample_end = desc.sample_count;
    req.seed = seed;
    req.mode = NH_MODE_MEGAKERNEL;
    req.traversal = traversal;
    req.clear = 1;
    auto t2 = std::chrono::steady_clock::now();
    if (nh_render(ctx, &req)) return die("render", nh_last_error(ctx));
    nh_synchronize(ctx);
    auto t3 = std::chrono::steady_clock::now();
    // Denoiser::denoise on the master block after the render loop (render.cpp:368-369)
    if (desc.denoiser.type != NH_DENOISER_NONE && nh_denoise(ctx, &desc.denoiser))
        return die("denoise", nh_last_error(ctx));
    const int W = desc.camera.width, H = desc.camera.height, B = desc.filter.border;
    std::vector<float> rgbw(4 * (size_t)(W + 2 * B) * (H + 2 * B)), rgb(3 * (size_t)W * H);
    nh_get_framebuffer(ctx, rgbw.data(), rgbw.size());
    nh_framebuffer_to_rgb(rgbw.data(), W, H, B, rgb.data());
    std::string out = scene_path;
    auto dot = out.find_last_of('.');
    if (dot != std::string::npos) out = out.substr(0, dot);
    if (png) nh_write_png((out + ".png").c_str(), rgb.data(), W, H);
    out += ".exr";
    nh_write_exr(out.c_str(), rgb.data(), W, H);
    if (!pfm.empty()) nh_write_pfm(pfm.c_str(), rgb.data(), W, H);
    double placed = (double)W * H * desc.sample_count;
    if (desc.sampler == NH_SAMPLER_ADAPTIVE) {
        // render.cpp:373 and :392-413: the samples the passes placed, and <scene>_variance.exr. The reference writes
        // every block's m_oldVariance v as Color4f(v) -- weight v -- through toBitmap's divideByFilterWeight, so
        // the file holds v / v where |v| > Epsilon and 0 elsewhere
        nh_adaptive_stats as;
        if (nh_get_adaptive_stats(ctx, &as)) return die("adaptive stats", nh_last_error(ctx));
        std::printf("Total Samples Placed: %llu\n", (unsigned long long)as.total_samples);
        placed = (double)as.total_samples;
        std::vector<float> var((size_t)W * H), vrgb(3 * (size_t)W * H);
        if (nh_get_adaptive_variance(ctx, var.data(), var.size())) return die("adaptive variance", nh_last_error(ctx));
        for (size_t i = 0; i < var.size(); ++i) {
            const float v = var[i], o = (v > 1e-4f || v < -1e-4f) ? v / v : 0.f;
            vrgb[3 * i] = vrgb[3 * i + 1] = vrgb[3 * i + 2] = o;
        }
        const std::string vout = out.substr(0, out.size() - 4) + "_variance.exr";
        nh_write_exr(vout.c_str(), vrgb.data(), W, H);
    }
    double bvh_s = std::chrono::duration<double>(t1 - t0).count();
    double rs = std::chrono::duration<double>(t3 - t2).count();
    double msps = placed / rs / 1e6;
    std::printf("nori_hip: %dx%d %d spp, BVH %u nodes (%.3f s), render %.3f s = %.2f Msamples/s -> %s\n", W, H,
                desc.sample_count, bd.n_nodes, bvh_s, rs, msps, out.c_str());
    nh_destroy(ctx);
    nh_bvh_free(bvh);
    nh_scene_free(scene);
    return 0;
}
