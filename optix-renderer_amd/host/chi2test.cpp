// hypothesis::chi2_test (ext/hypothesis/hypothesis.h:140-235) restated: the cells sorted by expected frequency, the
// two pooling branches, Pearson's statistic, the chi^2 tail, the Sidak-corrected level and the verdict. The
// distribution function is this file's own: chi2_cdf(x, dof) is the regularized lower incomplete gamma function
// P(dof / 2, x / 2), by its power series (DLMF 8.11.4) below the mode and by the continued fraction of Q = 1 - P
// (DLMF 8.9.2, modified Lentz) above it; dof == 2 keeps the reference's closed form.
//
// The sort: the reference's std::sort leaves the order of equal expected frequencies unspecified. Here it is the
// expected frequency, then the cell index; a NaN sorts last, so that the comparison stays an order.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "nh_host.h"

namespace {

// exp(a ln x - x - ln Gamma(a)) in long double: at a = 4096 the three terms are 3e4 each
double gamma_front(double a, double x) {
    return (double)std::exp((long double)a * std::log((long double)x) - (long double)x - std::lgamma((long double)a));
}

// P(a, x), a > 0
double gamma_p(double a, double x) {
    if (std::isnan(x)) return x;
    if (x <= 0.0) return 0.0;
    if (std::isinf(x)) return 1.0;
    const double eps = std::numeric_limits<double>::epsilon();
    if (x < a + 1.0) {  // sum over n of x^n / (a (a + 1) .. (a + n))
        double term = 1.0 / a, sum = term;
        for (int n = 1; n <= 1000000; ++n) {
            term *= x / (a + n);
            sum += term;
            if (term < sum * eps) break;
        }
        return std::min(1.0, gamma_front(a, x) * sum);
    }
    const double tiny = 1e-300;
    const auto guard = [&](double v) { return std::fabs(v) < tiny ? tiny : v; };
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / guard(b), h = d;
    for (int i = 1; i <= 1000000; ++i) {
        const double an = -(double)i * ((double)i - a);
        b += 2.0;
        d = 1.0 / guard(an * d + b);
        c = guard(b + an / c);
        const double step = d * c;
        h *= step;
        if (std::fabs(step - 1.0) < 4.0 * eps) break;
    }
    return 1.0 - gamma_front(a, x) * h;
}

// hypothesis.h:43-51
double chi2_cdf(double x, int dof) {
    if (dof < 1 || x < 0) return 0.0;
    if (dof == 2) return 1.0 - std::exp(-0.5 * x);
    return gamma_p(0.5 * dof, 0.5 * x);
}

}  // namespace

extern "C" int nh_chi2_test(int32_t n_cells, const double *obs, const double *exp, int32_t sample_count,
                            double min_exp_frequency, double alpha, int32_t num_tests, int32_t *accepted,
                            double *p_value, double *statistic, int32_t *dof_out, int32_t *pooled_out, int32_t *kind) {
    if (!accepted || !obs || !exp) { nh::set_host_error("nh_chi2_test: null argument"); return NH_ERR_INVALID; }
    if (n_cells < 1 || num_tests < 1) {
        nh::set_host_error("nh_chi2_test: needs at least 1 cell and 1 test");
        return NH_ERR_INVALID;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const auto finish = [&](int ok, int k, double p, double stat, int dof, int pooled) {
        *accepted = ok;
        if (kind) *kind = k;
        if (p_value) *p_value = p;
        if (statistic) *statistic = stat;
        if (dof_out) *dof_out = dof;
        if (pooled_out) *pooled_out = pooled;
        return NH_OK;
    };
    std::vector<int32_t> order((size_t)n_cells);
    for (int32_t i = 0; i < n_cells; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        const double ea = exp[a], eb = exp[b];
        if (std::isnan(ea) || std::isnan(eb)) return !std::isnan(ea) && std::isnan(eb);
        return ea < eb;
    });
    double pooled_obs = 0, pooled_exp = 0, chsq = 0;
    int pooled = 0, dof = 0;
    for (const int32_t i : order) {
        if (exp[i] == 0) {
            if (obs[i] > sample_count * 1e-5) return finish(0, NH_CHI2_REJECTED_ZERO_CELL, nan, obs[i], 0, pooled);
        } else if (exp[i] < min_exp_frequency) {
            pooled_obs += obs[i];
            pooled_exp += exp[i];
            pooled++;
        } else if (pooled_exp > 0 && pooled_exp < min_exp_frequency) {
            pooled_obs += obs[i];
            pooled_exp += exp[i];
            pooled++;
        } else {
            const double diff = obs[i] - exp[i];
            chsq += (diff * diff) / exp[i];
            ++dof;
        }
    }
    if (pooled_exp > 0 || pooled_obs > 0) {
        const double diff = pooled_obs - pooled_exp;
        chsq += (diff * diff) / pooled_exp;
        ++dof;
    }
    dof -= 1;
    if (dof <= 0) return finish(0, NH_CHI2_REJECTED_DOF, nan, chsq, dof, pooled);
    const double pval = 1 - chi2_cdf(chsq, dof);
    const double level = 1.0 - std::pow(1.0 - alpha, 1.0 / num_tests);
    const bool rejected = pval < level || !std::isfinite(pval);
    return finish(rejected ? 0 : 1, rejected ? NH_CHI2_REJECTED_P_VALUE : NH_CHI2_ACCEPTED, pval, chsq, dof, pooled);
}
