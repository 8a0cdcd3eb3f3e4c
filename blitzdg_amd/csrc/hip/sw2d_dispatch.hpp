// sw2d_dispatch.hpp -- host code only, no kernel headers: the run-time to compile-time dispatchers of the sw2d solvers.
// forOrder maps a polynomial order to a constant (which per-order launcher); the mode dispatchers map a stage mode, and where
// the kernels take it the filter flag, to constants (which kernel instance of a per-order file). Each calls a generic callable
// with std::integral_constant / std::bool_constant arguments exactly once and returns what it returns, so a kernel is
// instantiated only where the callable is; what no instance serves is hipErrorInvalidValue. tests/dispatch_check.cpp pins
// the instance sets.
#pragma once
#include <hip/hip_runtime_api.h>
#include <type_traits>
#include <utility>

namespace bdg_dev {

// The mode numbers of the kernel families, as their kernel headers name them (the per-order files assert the match): StageMode
// (sw2d_kernels.hpp) and CMODE_* (sw2d_curved_kernel.hpp) share one numbering, QuadMode (sw2d_quad_kernel.hpp) has its own.
struct TriModes { static constexpr int RHS = 0, LSERK = 1, COMBINE = 2; };
struct QuadModes { static constexpr int RHS = 0, COMBINE = 1, LSERK = 2, HEUN = 3; };

namespace dispatch_detail {
template <int M> using Mode = std::integral_constant<int, M>;

template <class F, int... I>
hipError_t forOrder(int order, F&& f, std::integer_sequence<int, I...>) {
    hipError_t e = hipErrorInvalidValue;
    (void)((order == I + 1 && ((e = f(Mode<I + 1>{})), true)) || ...);
    return e;
}

// The one rule set: RHS and COMBINE plain and filtered; LSERK plain, and filtered where LSERK_FILTERED; M::HEUN plain and
// filtered where HEUN.
template <class M, bool LSERK_FILTERED, bool HEUN, class F>
hipError_t forModeFilter(int mode, bool filter, F&& f) {
    auto either = [&](auto m) { return filter ? f(m, std::true_type{}) : f(m, std::false_type{}); };
    if (mode == M::RHS) return either(Mode<M::RHS>{});
    if (mode == M::COMBINE) return either(Mode<M::COMBINE>{});
    if (mode == M::LSERK) {
        if constexpr (LSERK_FILTERED) return either(Mode<M::LSERK>{});
        else return filter ? hipErrorInvalidValue : f(Mode<M::LSERK>{}, std::false_type{});
    }
    if constexpr (HEUN) {
        if (mode == M::HEUN) return either(Mode<M::HEUN>{});
    }
    return hipErrorInvalidValue;
}
} // namespace dispatch_detail

// f(std::integral_constant<int, order>) for an order in 1..MAX
template <int MAX, class F>
hipError_t forOrder(int order, F&& f) {
    return dispatch_detail::forOrder(order, std::forward<F>(f), std::make_integer_sequence<int, MAX>{});
}

// Straight-sided triangles, kernels without a filter flag: f(std::integral_constant<int, MODE>) for RHS, LSERK, COMBINE
template <class F>
hipError_t forMode(int mode, F&& f) {
    return dispatch_detail::forModeFilter<TriModes, true, false>(mode, false, [&](auto m, auto) { return f(m); });
}

// Straight-sided triangles: f(std::integral_constant<int, MODE>, std::bool_constant<FILT>); LSERK4 stages are unfiltered
template <class F>
hipError_t forModeFilter(int mode, bool filter, F&& f) {
    return dispatch_detail::forModeFilter<TriModes, false, false>(mode, filter, std::forward<F>(f));
}

// Curved triangles: every mode plain and filtered
template <class F>
hipError_t curvedForMode(int mode, bool filter, F&& f) {
    return dispatch_detail::forModeFilter<TriModes, true, false>(mode, filter, std::forward<F>(f));
}

// Quadrilaterals: RHS and COMBINE plain and filtered, LSERK plain, and with HEUN (variant B) QMODE_HEUN plain and filtered
template <bool HEUN, class F>
hipError_t quadForMode(int mode, bool filter, F&& f) {
    return dispatch_detail::forModeFilter<QuadModes, false, HEUN>(mode, filter, std::forward<F>(f));
}

} // namespace bdg_dev
