// The iterative adaptive Simpson rule (csrc/nh_simpson.h), host build, against the recursion it stands for written out
// plainly: results bit-identical, evaluation counts equal. No HIP. Run by tests/test_simpson_host.py; prints one line
// per case and exits non-zero at the first mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>

#include "nh_simpson.h"

namespace {

using Fn = std::function<double(double)>;

// one interval [a, c] with midpoint b: refine, then stop by Lyness' criterion or split into [a, b] and [b, c]
double refine(const Fn &f, double a, double b, double c, double fa, double fb, double fc, double I, double eps, int depth,
              long &leaves) {
    const double d = 0.5f * (a + b), e = 0.5f * (b + c);
    const double fd = f(d);
    const double fe = f(e);
    const double h = c - a;
    const double I0 = (1.0 / 12.0) * h * (fa + 4.0 * fd + fb);
    const double I1 = (1.0 / 12.0) * h * (fb + 4.0 * fe + fc);
    const double Ip = I0 + I1;
    if (depth <= 0 || std::abs(Ip - I) < 15.0 * eps) {
        ++leaves;
        return Ip + (1.0 / 15.0) * (Ip - I);
    }
    const double left = refine(f, a, d, b, fa, fd, fb, I0, 0.5 * eps, depth - 1, leaves);
    const double right = refine(f, b, e, c, fb, fe, fc, I1, 0.5 * eps, depth - 1, leaves);
    return left + right;
}

double recursive_simpson(const Fn &f, double x0, double x1, double eps, int depth, long &leaves) {
    const double a = x0, b = 0.5 * (x0 + x1), c = x1;
    const double fa = f(a);
    const double fb = f(b);
    const double fc = f(c);
    const double I = (c - a) * (1.0 / 6.0) * (fa + 4.0 * fb + fc);
    return refine(f, a, b, c, fa, fb, fc, I, eps, depth, leaves);
}

bool same_bits(double x, double y) {
    uint64_t a, b;
    std::memcpy(&a, &x, 8);
    std::memcpy(&b, &y, 8);
    return a == b || (std::isnan(x) && std::isnan(y));
}

int failures = 0;

// want_leaves < 0: not checked
void check_1d(const char *name, const Fn &f, double x0, double x1, double eps, int depth, long want_leaves) {
    long evals_rec = 0, evals_it = 0, leaves = 0;
    const double rec = recursive_simpson([&](double x) { ++evals_rec; return f(x); }, x0, x1, eps, depth, leaves);
    const double it = nhd::adaptive_simpson([&](double x) { ++evals_it; return f(x); }, x0, x1, eps, depth);
    const bool ok = same_bits(rec, it) && evals_rec == evals_it && (want_leaves < 0 || leaves == want_leaves);
    std::printf("%s: %.17g %s, %ld evaluations, %ld leaves\n", name, it, ok ? "OK" : "MISMATCH", evals_it, leaves);
    if (!ok) {
        std::printf("  recursion: %.17g, %ld evaluations (leaves wanted: %ld)\n", rec, evals_rec, want_leaves);
        ++failures;
    }
}

void check_2d(const char *name, const std::function<double(double, double)> &f, double x0, double y0, double x1,
              double y1) {
    long evals_rec = 0, evals_it = 0, leaves = 0;
    const double rec = recursive_simpson(
        [&](double y) {
            return recursive_simpson([&](double x) { ++evals_rec; return f(x, y); }, x0, x1, 1e-6, 6, leaves);
        },
        y0, y1, 1e-6, 6, leaves);
    const double it = nhd::adaptive_simpson_2d([&](double x, double y) { ++evals_it; return f(x, y); }, x0, y0, x1, y1);
    const bool ok = same_bits(rec, it) && evals_rec == evals_it;
    std::printf("%s: %.17g %s, %ld evaluations\n", name, it, ok ? "OK" : "MISMATCH", evals_it);
    if (!ok) {
        std::printf("  recursion: %.17g, %ld evaluations\n", rec, evals_rec);
        ++failures;
    }
}

}  // namespace

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // Simpson's rule is exact on a cubic: the first refinement already agrees, one leaf
    check_1d("cubic", [](double x) { return ((2.0 * x - 1.0) * x + 0.5) * x - 3.0; }, -1.0, 2.0, 1e-6, 6, 1);
    // the depth limit ends every branch: 2^6 leaves below the first refinement's two halves
    check_1d("gaussian", [](double x) { return 1e9 * std::exp(-0.5 * (x - 0.37) * (x - 0.37) / (0.15 * 0.15)); }, 0.0,
             1.0, 1e-6, 6, 64);
    // a narrower one is refined around its peak only
    check_1d("narrow", [](double x) { return std::exp(-0.5 * (x - 0.37) * (x - 0.37) / (0.05 * 0.05)); }, 0.0, 1.0,
             1e-6, 6, -1);
    check_1d("rough", [](double x) { return 1e3 * std::sin(1e4 * x * x); }, 0.0, 1.0, 1e-6, 6, 64);
    check_1d("step", [](double x) { return x < 0.3 ? 0.0 : 1.0; }, 0.0, 1.0, 1e-6, 6, -1);
    check_1d("zero", [](double) { return 0.0; }, 0.0, 1.0, 1e-6, 6, 1);
    check_1d("nan", [nan](double) { return nan; }, 0.0, 1.0, 1e-6, 6, 64);
    check_1d("nan-in-part", [nan](double x) { return x > 0.8 ? nan : x * x; }, 0.0, 1.0, 1e-6, 6, -1);
    for (int depth = -1; depth <= 6; ++depth) {
        char name[32];
        std::snprintf(name, sizeof(name), "depth %d", depth);
        check_1d(name, [](double x) { return 1e3 * std::sin(1e4 * x * x); }, 0.0, 1.0, 1e-6, depth,
                 depth <= 0 ? 1 : 1L << depth);
    }
    check_1d("reversed", [](double x) { return std::exp(x); }, 1.0, 0.0, 1e-9, 6, -1);
    check_1d("tight", [](double x) { return std::sqrt(x); }, 0.0, 1.0, 1e-12, 6, -1);
    // the nested form: a narrow lobe in a cell, a discontinuity across it, and nothing at all
    check_2d("2d lobe", [](double x, double y) { return std::exp(-40.0 * ((x - 0.3) * (x - 0.3) + (y - 1.1) * (y - 1.1))); },
             0.0, 0.0, 1.0, 2.0);
    check_2d("2d step", [](double x, double y) { return x + 0.5 * y < 0.9 ? 0.0 : x * y; }, 0.0, 0.0, 1.0, 2.0);
    check_2d("2d zero", [](double, double) { return 0.0; }, -1.0, 0.0, -0.8, 0.3);
    check_2d("2d nan", [nan](double x, double) { return x > 0.5 ? nan : 1.0; }, 0.0, 0.0, 1.0, 1.0);
    if (failures) {
        std::printf("simpson_check: %d MISMATCHES\n", failures);
        return 1;
    }
    std::printf("simpson_check: all cases OK\n");
    return 0;
}
