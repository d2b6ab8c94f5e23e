// CPU check of the launchers' dispatch helpers (optix-renderer_amd/csrc/nh_dispatch.h), run by
// tests/test_dispatch_host.py. Plain C++17: the header has no HIP in it.
//
//   nh_dispatch        for 1 to 5 flags and each of the 2^n run-time combinations: the callee runs exactly once, with
//                      constants equal to the run-time values, in argument order
//   nh_dispatch_depth  for each bucket list the launchers use (and the two halves of the wavefront traversal
//                      launchers' chain): every boundary value lands in the bucket the `<=` chain gives
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "nh_dispatch.h"

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            ++failures;                   \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");            \
        }                                 \
    } while (0)

// flag j of combination c of n flags (any numbering that visits every combination)
static bool bit(unsigned c, int j) { return (c >> j) & 1u; }

// one nh_dispatch call over `want`; the callee records how often it ran and what it received
template <class... B>
static void check_flags(unsigned c, B... want) {
    const bool expect[] = {want...};
    const int n = (int)sizeof...(B);
    int calls = 0;
    std::vector<bool> got;
    nh_dispatch(
        [&](auto... k) {
            ++calls;
            // each argument is a compile-time constant: usable as a template argument
            got = {std::bool_constant<decltype(k)::value>::value...};
            static_assert(sizeof...(k) == sizeof...(B), "one constant per flag");
        },
        want...);
    CHECK(calls == 1, "%d flags, combination %u: %d calls", n, c, calls);
    CHECK((int)got.size() == n, "%d flags, combination %u: %d constants", n, c, (int)got.size());
    for (int j = 0; j < n && j < (int)got.size(); ++j)
        CHECK(got[j] == expect[j], "%d flags, combination %u: flag %d arrived as %d", n, c, j, (int)got[j]);
}

static int check_all_flags() {
    int combos = 0;
    for (unsigned c = 0; c < 2; ++c, ++combos) check_flags(c, bit(c, 0));
    for (unsigned c = 0; c < 4; ++c, ++combos) check_flags(c, bit(c, 0), bit(c, 1));
    for (unsigned c = 0; c < 8; ++c, ++combos) check_flags(c, bit(c, 0), bit(c, 1), bit(c, 2));
    for (unsigned c = 0; c < 16; ++c, ++combos) check_flags(c, bit(c, 0), bit(c, 1), bit(c, 2), bit(c, 3));
    for (unsigned c = 0; c < 32; ++c, ++combos) check_flags(c, bit(c, 0), bit(c, 1), bit(c, 2), bit(c, 3), bit(c, 4));
    return combos;
}

// the bucket an if chain `if (depth <= b0) .. else if (depth <= b1) .. else last` gives
static int chain_bucket(int depth, std::initializer_list<int> buckets) {
    int last = 0;
    for (int b : buckets) {
        if (depth <= b) return b;
        last = b;
    }
    return last;
}

template <int... Ds>
static int check_depth_list() {
    int n = 0;
    for (int depth : {0, 1, 16, 17, 32, 33, 64, 65, 128, 129, 1000}) {
        int calls = 0, got = -1;
        nh_dispatch_depth<Ds...>(depth, [&](auto d) {
            ++calls;
            got = std::integral_constant<int, decltype(d)::value>::value;
        });
        const int want = chain_bucket(depth, {Ds...});
        CHECK(calls == 1, "depth %d: %d calls", depth, calls);
        CHECK(got == want, "depth %d: bucket %d, the chain gives %d", depth, got, want);
        ++n;
    }
    return n;
}

int main() {
    const int combos = check_all_flags();
    int depths = 0;
    depths += check_depth_list<16, 32, 64, 128>();  // launch_trace, launch_path, launch_wf_tail
    depths += check_depth_list<32, 64, 128>();      // launch_vol_path, launch_adaptive_paths
    depths += check_depth_list<16, 32>();           // (the halves the wavefront traversal launchers keep as if chains)
    depths += check_depth_list<64, 128>();
    // the chain itself, spelled out once
    CHECK(chain_bucket(16, {16, 32, 64, 128}) == 16 && chain_bucket(17, {16, 32, 64, 128}) == 32 &&
              chain_bucket(129, {16, 32, 64, 128}) == 128 && chain_bucket(16, {32, 64, 128}) == 32,
          "chain_bucket");
    std::printf("%d flag combinations, %d depth values, %d failures\n", combos, depths, failures);
    return failures ? 1 : 0;
}
