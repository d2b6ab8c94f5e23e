// hypothesis::students_t_test (ext/hypothesis/hypothesis.h:314-346) restated: the statistic, the two-sided p-value of
// Student's t, the Sidak-corrected level and the verdict. The distribution function is this file's own: for nu degrees
// of freedom the two-sided tail P(|T| > t) is the regularized incomplete beta function I_x(nu / 2, 1 / 2) at
// x = nu / (nu + t^2), evaluated by its continued fraction (DLMF 8.17.22) with the modified Lentz recurrence, on the
// side of the symmetry I_x(a, b) = 1 - I_{1-x}(b, a) where the fraction converges fast.
#include <algorithm>
#include <cmath>
#include <limits>

#include "nh_host.h"

namespace {

// The continued fraction of I_x(a, b) without its front factor: 1 / (1 + d1 / (1 + d2 / (1 + ..)))
double beta_fraction(double a, double b, double x) {
    const double tiny = 1e-300, eps = 4.0 * std::numeric_limits<double>::epsilon();
    const auto guard = [&](double v) { return std::fabs(v) < tiny ? tiny : v; };
    double c = 1.0, d = 1.0 / guard(1.0 - (a + b) * x / (a + 1.0)), h = d;
    for (int m = 1; m <= 200000; ++m) {
        const double m2 = 2.0 * m;
        // d_{2m}
        double num = m * (b - m) * x / ((a + m2 - 1.0) * (a + m2));
        d = 1.0 / guard(1.0 + num * d);
        c = guard(1.0 + num / c);
        h *= d * c;
        // d_{2m+1}
        num = -(a + m) * (a + b + m) * x / ((a + m2) * (a + m2 + 1.0));
        d = 1.0 / guard(1.0 + num * d);
        c = guard(1.0 + num / c);
        const double step = d * c;
        h *= step;
        if (std::fabs(step - 1.0) < eps) break;
    }
    return h;
}

// I_x(a, b) with y = 1 - x given separately (either may be tiny). ln B(a, b) in long double: at a = 5e4 the
// three lgamma terms are 5e5 each and their difference is the exponent of the front factor
double beta_regularized(double a, double b, double x, double y) {
    if (x <= 0.0) return 0.0;
    if (y <= 0.0) return 1.0;
    const long double lbeta = std::lgamma((long double)a) + std::lgamma((long double)b) - std::lgamma((long double)a + (long double)b);
    const double lx = x < 0.5 ? std::log(x) : std::log1p(-y), ly = y < 0.5 ? std::log(y) : std::log1p(-x);
    const double front = std::exp((double)((long double)a * lx + (long double)b * ly - lbeta));
    if (x < (a + 1.0) / (a + b + 2.0)) return front * beta_fraction(a, b, x) / a;
    return 1.0 - front * beta_fraction(b, a, y) / b;
}

// P(|T| > t) for Student's t with nu degrees of freedom, t >= 0
double students_t_two_sided(double t, double nu) {
    if (std::isnan(t)) return t;
    if (std::isinf(t)) return 0.0;
    const double t2 = t * t, s = nu + t2;
    return beta_regularized(0.5 * nu, 0.5, nu / s, t2 / s);
}

}  // namespace

extern "C" int nh_students_t_test(double mean, double variance, double reference, int32_t n, double alpha,
                                  int32_t num_tests, int32_t *accepted, double *p_value) {
    if (!accepted) { nh::set_host_error("nh_students_t_test: null argument"); return NH_ERR_INVALID; }
    if (n < 2 || num_tests < 1) {
        nh::set_host_error("nh_students_t_test: needs at least 2 samples and 1 test");
        return NH_ERR_INVALID;
    }
    const double t = std::fabs(mean - reference) * std::sqrt((double)n / std::max(variance, 1e-5));
    const double pval = students_t_two_sided(t, (double)(n - 1));
    const double level = 1.0 - std::pow(1.0 - alpha, 1.0 / (double)num_tests);
    *accepted = (pval < level || !std::isfinite(pval)) ? 0 : 1;
    if (p_value) *p_value = pval;
    return NH_OK;
}
