// Run-time value -> template argument, for the launchers of the scan kernels.  A kernel family keeps the run-time
// values of its template parameters in one struct, says in one constexpr `..._built()` predicate which combinations
// exist in the binary, and its launcher nests these two lifts over the struct's fields.  Both return
// what f returns: true = a kernel was launched.
#pragma once
#include "common.h"
#include <type_traits>

namespace fastgrnn {
namespace {

template <typename Fn> __attribute__((always_inline)) inline bool pick_bool(bool v, Fn&& f) {
  return v ? f(std::true_type{}) : f(std::false_type{});
}
// f(std::integral_constant<int, V>{}) for the V that equals v; false if none does
template <int... Vs, typename Fn> __attribute__((always_inline)) inline bool pick_int(int v, Fn&& f) {
  return ((v == Vs && f(std::integral_constant<int, Vs>{})) || ...);
}

static_assert(FASTGRNN_NL_SIGMOID == 0 && FASTGRNN_NL_RELU == 1 && FASTGRNN_NL_TANH == 2 && FASTGRNN_NL_QUANT_TANH == 3 &&
              FASTGRNN_NL_QUANT_SIGM == 4 && FASTGRNN_NL_QUANT_SIGM4 == 5, "pick_int<0, 1, 2[, 3, 4, 5]>(d.gate_nl, ...)");

// gates that keep z in [0,1] and so bound the growth of h to sigma(nu) per step: the ones the fp16 two-plane state
// product of the forward scans is built for (see fwd_scan_split_w8)
constexpr bool gate_bounds_state(int gate) {
  return gate == FASTGRNN_NL_SIGMOID || gate == FASTGRNN_NL_QUANT_SIGM || gate == FASTGRNN_NL_QUANT_SIGM4;
}

}  // namespace
}  // namespace fastgrnn
