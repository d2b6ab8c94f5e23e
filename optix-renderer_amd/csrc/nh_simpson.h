// hypothesis::adaptiveSimpson and adaptiveSimpson2D (ext/hypothesis/hypothesis.h:62-102) without recursion: Lyness'
// criterion |Ip - I| < 15 eps with eps halved per level, Richardson's term Ip + (Ip - I) / 15 at a leaf, and the
// partial sums combined in the recursion's own tree order (left + right, post-order), so the result has the bits the
// recursive form gives. Plain C++, compiled for host and device: tests/c/simpson_check.cpp checks the host build
// against the recursion written out.
//
// The walk keeps one frame per level on an explicit stack: `depth` levels of refinement below the first need
// depth + 1 frames, and a deeper request than NH_SIMPSON_MAX_DEPTH is cut to it. A frame is evaluated once (its two
// midpoints, d before e), then either returns as a leaf or waits for its left and then its right child. An integrand
// that returns NaN never meets the criterion and ends at the depth limit, 2^depth leaf frames of two panels each.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NH_SIMPSON_HD __host__ __device__
#else
#define NH_SIMPSON_HD
#endif

#define NH_SIMPSON_MAX_DEPTH 6

namespace nhd {

struct SimpsonFrame {
    double a, b, c, fa, fb, fc, I, eps;  // the interval [a, c], its midpoint b, the values there, Simpson's rule on it
    double d, e, fd, fe, I0, I1;         // the two halves, filled when the frame is evaluated
    double left;                         // the left child's result, while the right one runs
    int depth, phase;                    // phase 0: not evaluated; 1: the left child runs; 2: the right child runs
};

// the integral of f over [x0, x1]; f: double -> double
template <class F>
NH_SIMPSON_HD inline double adaptive_simpson(F &&f, double x0, double x1, double eps = 1e-6,
                                             int depth = NH_SIMPSON_MAX_DEPTH) {
    SimpsonFrame st[NH_SIMPSON_MAX_DEPTH + 1];
    if (depth > NH_SIMPSON_MAX_DEPTH) depth = NH_SIMPSON_MAX_DEPTH;
    {
        SimpsonFrame &r = st[0];
        r.a = x0;
        r.b = 0.5 * (x0 + x1);
        r.c = x1;
        r.fa = f(r.a);
        r.fb = f(r.b);
        r.fc = f(r.c);
        r.I = (r.c - r.a) * (1.0 / 6.0) * (r.fa + 4.0 * r.fb + r.fc);
        r.eps = eps;
        r.depth = depth;
        r.phase = 0;
    }
    int sp = 1;  // frames in use; st[sp - 1] is the one at work
    double ret = 0.0;
    while (sp > 0) {
        SimpsonFrame &t = st[sp - 1];
        bool returned = false;
        if (t.phase == 0) {
            t.d = 0.5f * (t.a + t.b);
            t.e = 0.5f * (t.b + t.c);
            t.fd = f(t.d);
            t.fe = f(t.e);
            const double h = t.c - t.a;
            t.I0 = (1.0 / 12.0) * h * (t.fa + 4.0 * t.fd + t.fb);
            t.I1 = (1.0 / 12.0) * h * (t.fb + 4.0 * t.fe + t.fc);
            const double Ip = t.I0 + t.I1, diff = Ip - t.I;
            if (t.depth <= 0 || (diff < 0 ? -diff : diff) < 15.0 * t.eps) {
                ret = Ip + (1.0 / 15.0) * diff;
                returned = true;
                --sp;
            } else {  // (t.depth >= 1 here, so sp <= depth <= NH_SIMPSON_MAX_DEPTH: the child's frame exists)
                t.phase = 1;
                SimpsonFrame &l = st[sp++];
                l.a = t.a; l.b = t.d; l.c = t.b;
                l.fa = t.fa; l.fb = t.fd; l.fc = t.fb;
                l.I = t.I0;
                l.eps = 0.5 * t.eps;
                l.depth = t.depth - 1;
                l.phase = 0;
            }
        }
        // hand a finished frame's value to its parent: the left value waits, the right one completes the sum
        while (returned && sp > 0) {
            SimpsonFrame &p = st[sp - 1];
            if (p.phase == 1) {
                p.left = ret;
                p.phase = 2;
                SimpsonFrame &r = st[sp++];
                r.a = p.b; r.b = p.e; r.c = p.c;
                r.fa = p.fb; r.fb = p.fe; r.fc = p.fc;
                r.I = p.I1;
                r.eps = 0.5 * p.eps;
                r.depth = p.depth - 1;
                r.phase = 0;
                returned = false;
            } else {
                ret = p.left + ret;
                --sp;
            }
        }
    }
    return ret;
}

// the integral of f(x, y) over [x0, x1] x [y0, y1]: the outer rule runs over y, and every y node integrates over x
template <class F>
NH_SIMPSON_HD inline double adaptive_simpson_2d(F &&f, double x0, double y0, double x1, double y1, double eps = 1e-6,
                                                int depth = NH_SIMPSON_MAX_DEPTH) {
    return adaptive_simpson(
        [&](double y) { return adaptive_simpson([&](double x) { return f(x, y); }, x0, x1, eps, depth); }, y0, y1, eps,
        depth);
}

}  // namespace nhd
