// The combine step of the flat two-leaf traversal (nh_traverse.h trace_flat): from each leaf's own best hit, found
// against the query's entry maxt, the answer the stack walk of trace() gives. Plain C++, compiled for host and device:
// tests/c/flat_combine_check.cpp checks the host build against an in-order two-leaf loop.
//
// Why a leaf's best can be found before the other leaf's is known: a record's candidate t does not depend on maxt, and
// the acceptance rule (t <= maxt, replacing on t < maxt or a later record) keeps, after any order of tests, the
// smallest candidate, ties to the largest record index. So the leaf's best against the entry maxt is its best against
// any smaller maxt' too when it passes t <= maxt', and when it does not the leaf holds no candidate that does. What
// depends on the order is only whether the second leaf is visited at all: trace() re-tests its box when it pops it,
// and of that test's three terms only near <= maxt depends on maxt.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NH_FLAT_HD __host__ __device__ __forceinline__
#else
#define NH_FLAT_HD inline
#endif

namespace nhd {

// a leaf's best hit: the smallest accepted t, ties to the largest record index k; found false: none (k = -1)
struct FlatBest {
    float t, u, v;
    int k;
    bool found;
};

// hl, hr: the child boxes' tests against the entry maxt; nl, nr: their entry distances. L, R: the leaves' bests against
// the entry maxt (of a leaf whose box missed: anything). Returns found; the hit in out.
template <bool ORDERED>
NH_FLAT_HD bool flat_combine(bool hl, bool hr, float nl, float nr, float maxt, const FlatBest &L, const FlatBest &R,
                             FlatBest &out) {
    const bool both = hl && hr;
    const bool right_first = both ? (ORDERED && nr < nl) : hr;  // the child visited first (one hit box: that one)
    const FlatBest &F = right_first ? R : L, &S = right_first ? L : R;
    const bool found_first = (hl || hr) && F.found;
    const float maxt1 = found_first ? F.t : maxt;
    const int k_first = found_first ? F.k : -1;
    // the deferred child's pop-time box test, then its best under the acceptance rule with the first's as the best
    const float near_second = right_first ? nl : nr;
    const bool take_second = both && near_second <= maxt1 && S.found && S.t <= maxt1 && (S.t < maxt1 || S.k > k_first);
    out.t = take_second ? S.t : F.t;
    out.u = take_second ? S.u : F.u;
    out.v = take_second ? S.v : F.v;
    out.k = take_second ? S.k : k_first;
    out.found = found_first || take_second;
    return out.found;
}

// any hit: maxt never shrinks, so each leaf whose box hit answers for itself
NH_FLAT_HD bool flat_combine_any(bool hl, bool hr, bool any_l, bool any_r) { return (hl && any_l) || (hr && any_r); }

}  // namespace nhd
