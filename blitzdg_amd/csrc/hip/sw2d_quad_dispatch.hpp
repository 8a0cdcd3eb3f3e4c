// sw2d_quad_dispatch.hpp -- host code only: the two run-time to compile-time dispatchers of the quadrilateral sw2d
// solver. quadForOrder maps the order to a constant (sw2d_quad_device.hip: which per-order launcher); quadForMode maps
// (mode, filter) to constants (the per-order files sw2d_quad*_order.hip: which kernel instance). Each calls a generic
// callable with std::integral_constant arguments, so a kernel is instantiated only where the callable is.
#pragma once
#include "sw2d_quad_kernel.hpp"
#include <type_traits>
#include <utility>

namespace bdg_dev {

namespace quad_dispatch_detail {
template <class F, int... I>
hipError_t forOrder(int order, F&& f, std::integer_sequence<int, I...>) {
    hipError_t e = hipErrorInvalidValue;
    (void)((order == I + 1 && ((e = f(std::integral_constant<int, I + 1>{})), true)) || ...);
    return e;
}
} // namespace quad_dispatch_detail

// f(std::integral_constant<int, order>) for an order in 1..MAX; hipErrorInvalidValue outside
template <int MAX, class F>
hipError_t quadForOrder(int order, F&& f) {
    return quad_dispatch_detail::forOrder(order, std::forward<F>(f), std::make_integer_sequence<int, MAX>{});
}

// f(std::integral_constant<int, MODE>, std::bool_constant<FILT>) for the instances that exist: RHS and COMBINE plain and
// filtered, LSERK plain (LSERK4 stages are unfiltered), and with HEUN (variant B) QMODE_HEUN plain and filtered;
// hipErrorInvalidValue for everything else
template <bool HEUN, class F>
hipError_t quadForMode(int mode, bool filter, F&& f) {
    auto either = [&](auto m) { return filter ? f(m, std::true_type{}) : f(m, std::false_type{}); };
    switch (mode) {
    case QMODE_RHS: return either(std::integral_constant<int, QMODE_RHS>{});
    case QMODE_COMBINE: return either(std::integral_constant<int, QMODE_COMBINE>{});
    case QMODE_LSERK:
        return filter ? hipErrorInvalidValue : f(std::integral_constant<int, QMODE_LSERK>{}, std::false_type{});
    case QMODE_HEUN:
        if constexpr (HEUN) return either(std::integral_constant<int, QMODE_HEUN>{});
        else return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
    }
}

} // namespace bdg_dev
