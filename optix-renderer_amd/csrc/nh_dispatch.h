// Choosing a template instantiation from run-time values, for the launchers. Plain C++17, no HIP:
// tests/c/dispatch_check.cpp compiles it with the host compiler alone.
#pragma once
#include <type_traits>

// nh_dispatch(f, b0, b1, ..): calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ..) once. f is a generic
// lambda; each flag arrives as a constant it can use as a template argument or under `if constexpr`:
//
//   nh_dispatch([&](auto O, auto T) { hipLaunchKernelGGL((kernel<O, T>), ..); }, ordered, stats);
//
// Every combination of the flags is instantiated, first flag outermost, `true` first; a combination that must not be
// built is fenced with `if constexpr` inside the lambda.
template <bool... Done, class F>
void nh_dispatch(F &&f) {
    f(std::bool_constant<Done>{}...);
}
template <bool... Done, class F, class... Rest>
void nh_dispatch(F &&f, bool b, Rest... rest) {
    if (b) nh_dispatch<Done..., true>(f, rest...);
    else nh_dispatch<Done..., false>(f, rest...);
}

// nh_dispatch_depth<D0, D1, ..>(depth, f): calls f(std::integral_constant<int, D>{}) for the first D of the ascending
// list with depth <= D; the last entry takes every deeper value as well, as the last `else` of an if chain does.
template <int D0, int... Ds, class F>
void nh_dispatch_depth(int depth, F &&f) {
    if constexpr (sizeof...(Ds) == 0) {
        f(std::integral_constant<int, D0>{});
    } else {
        if (depth <= D0) f(std::integral_constant<int, D0>{});
        else nh_dispatch_depth<Ds...>(depth, f);
    }
}
