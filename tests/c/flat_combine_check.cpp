// The combine step of the flat two-leaf traversal (csrc/nh_flat_combine.h), host build, against the walk it stands
// for written out: visit the first child's leaf, re-test the deferred child's entry distance against the maxt of that
// moment, visit it, every candidate accepted in order under trace()'s rule. No HIP. Run by
// tests/test_flat_combine_host.py; prints the number of cases and exits non-zero at the first mismatch.
#include <cmath>
#include <cstdio>
#include <vector>

#include "nh_flat_combine.h"

namespace {

struct Cand {
    float t;
    int k;
};
struct Best {
    float t = INFINITY;
    int k = -1;
    bool found = false;
};

// one leaf's records in order under the acceptance rule of leaf_test / accept_hit
void visit(const std::vector<Cand> &leaf, float &maxt, Best &best, bool &any) {
    for (const Cand &c : leaf) {
        if (!(c.t <= maxt)) continue;
        any = true;
        if (c.t < maxt || c.k > best.k) {
            maxt = c.t;
            best.t = c.t;
            best.k = c.k;
            best.found = true;
        }
    }
}

// trace() on a root with two leaves whose box tests against the entry maxt gave (hl, nl) and (hr, nr)
Best walk(bool ordered, bool hl, bool hr, float nl, float nr, float maxt, const std::vector<Cand> &L,
          const std::vector<Cand> &R, bool &any) {
    Best best;
    any = false;
    if (hl && hr) {
        const bool right_first = ordered && nr < nl;
        visit(right_first ? R : L, maxt, best, any);
        if ((right_first ? nl : nr) <= maxt) visit(right_first ? L : R, maxt, best, any);  // the pop-time re-test
    } else if (hl) {
        visit(L, maxt, best, any);
    } else if (hr) {
        visit(R, maxt, best, any);
    }
    return best;
}

// trace()'s any-hit walk: maxt does not shrink, the first accepted candidate answers
bool walk_any(bool hl, bool hr, float nr, float maxt, const std::vector<Cand> &L, const std::vector<Cand> &R) {
    const auto leaf_any = [&](const std::vector<Cand> &leaf) {
        for (const Cand &c : leaf)
            if (c.t <= maxt) return true;
        return false;
    };
    if (hl && hr) return leaf_any(L) || (nr <= maxt && leaf_any(R));
    return (hl && leaf_any(L)) || (hr && leaf_any(R));
}

nhd::FlatBest leaf_best(const std::vector<Cand> &leaf, float maxt, bool &any) {
    Best b;
    any = false;
    visit(leaf, maxt, b, any);
    // u, v stand for the record: the combine step must carry them with the k it picks
    return nhd::FlatBest{b.t, (float)b.k + 0.25f, (float)b.k + 0.5f, b.k, b.found};
}

}  // namespace

int main() {
    const float kMaxt = 3.f;
    const float ts[] = {-1.f, 1.f, 2.f, 3.f, 4.f};       // -1: the slot holds no candidate; 4 is past the entry maxt
    const float nears[] = {0.f, 1.f, 2.f, 3.f, 3.5f};    // 3.5: the box misses (near > maxt)
    long cases = 0;
    for (float l0 : ts) for (float l1 : ts) for (float r0 : ts) for (float r1 : ts) {
        std::vector<Cand> L, R;  // the left leaf holds records 0 and 1, the right one 2 and 3
        if (l0 > 0) L.push_back({l0, 0});
        if (l1 > 0) L.push_back({l1, 1});
        if (r0 > 0) R.push_back({r0, 2});
        if (r1 > 0) R.push_back({r1, 3});
        for (float nl : nears) for (float nr : nears)
            for (int hits = 0; hits < 4; ++hits) {
                const bool hl = (hits & 1) && nl <= kMaxt, hr = (hits & 2) && nr <= kMaxt;
                bool any_l, any_r, any_w;
                const nhd::FlatBest bl = leaf_best(L, kMaxt, any_l), br = leaf_best(R, kMaxt, any_r);
                for (int ordered = 0; ordered < 2; ++ordered) {
                    const Best w = walk(ordered != 0, hl, hr, nl, nr, kMaxt, L, R, any_w);
                    nhd::FlatBest out;
                    const bool found = ordered ? nhd::flat_combine<true>(hl, hr, nl, nr, kMaxt, bl, br, out)
                                               : nhd::flat_combine<false>(hl, hr, nl, nr, kMaxt, bl, br, out);
                    ++cases;
                    bool ok = found == w.found && out.found == w.found && out.k == w.k;
                    if (ok && w.found) ok = out.t == w.t && out.u == (float)w.k + 0.25f && out.v == (float)w.k + 0.5f;
                    if (!ok) {
                        std::printf("mismatch: ordered %d hl %d hr %d nl %g nr %g L (%g %g) R (%g %g): walk (%d %g %d) "
                                    "combine (%d %g %d)\n", ordered, hl, hr, nl, nr, l0, l1, r0, r1, w.found, w.t, w.k,
                                    out.found, out.t, out.k);
                        return 1;
                    }
                }
                ++cases;
                if (nhd::flat_combine_any(hl, hr, any_l, any_r) != walk_any(hl, hr, nr, kMaxt, L, R)) {
                    std::printf("any-hit mismatch: hl %d hr %d nl %g nr %g L (%g %g) R (%g %g)\n", hl, hr, nl, nr, l0, l1,
                                r0, r1);
                    return 1;
                }
            }
    }
    std::printf("flat_combine_check: %ld cases OK\n", cases);
    return 0;
}
