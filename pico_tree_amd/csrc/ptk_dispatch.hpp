// ptk_dispatch.hpp -- how the launch layer turns a run-time value into a template argument, written once.  Each helper
// picks a compile-time tag from one value and calls a generic lambda with it; what the lambda returns (an int status)
// comes back unchanged.  A kernel instantiation is added in ONE lambda body: the helpers instantiate it for every tag.
// Plain C++17: no HIP, no handle types -- the metric types of the kernel headers are only named here.
#pragma once

#include <cstdint>
#include <type_traits>
#include <utility>

#include "ptk.h"  // PTK_METRIC_*

namespace ptk {
struct MetricL2;  // ptk_kernels.hpp
struct MetricL1;
struct MetricLInf;
struct MetricLNInf;
struct TopoSO2;  // ptk_kernels_topo.hpp
struct TopoSE2;
struct Metric64L2;  // ptk_kernels_f64.hpp
struct Metric64L1;
struct Metric64LInf;
struct Metric64LNInf;
struct Topo64SO2;
struct Topo64SE2;
}  // namespace ptk

namespace ptkd {

template <int V>
using int_tag = std::integral_constant<int, V>;
template <class T>
struct type_tag {
  using type = T;
};
// `typename decltype(m)::type` of a lambda's tag argument.
template <class Tag>
using type_of = typename Tag::type;

// The k-list size: f(int_tag<V>) for the first V of the list with k <= V, the last V when k exceeds them all.
template <int V, int... Rest, class F>
int with_slots(uint32_t k, F&& f) {
  if constexpr (sizeof...(Rest) == 0) return f(int_tag<V>{});
  else return k <= (uint32_t)V ? f(int_tag<V>{}) : with_slots<Rest...>(k, std::forward<F>(f));
}

template <class F>
int with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
template <class F>
int with_bools(bool a, bool b, F&& f) {
  return with_bool(a, [&](auto A) { return with_bool(b, [&](auto B) { return f(A, B); }); });
}

// The private spill class: f(int_tag<Slots[cls]>); none() where cls names no entry of the list.
template <int V, int... Rest, class F, class G>
int with_ovf(int cls, F&& f, G&& none) {
  if (cls == 0) return f(int_tag<V>{});
  if constexpr (sizeof...(Rest) == 0) return none();
  else return with_ovf<Rest...>(cls - 1, std::forward<F>(f), std::forward<G>(none));
}

// The metric of a handle (a PTK_METRIC_* id): f(type_tag<M>), one function per set of metrics a path is compiled for.
template <class L2, class L1, class LInf, class LNInf, class F>
int with_euclid_of(int id, F&& f) {
  switch (id) {
    case PTK_METRIC_L1: return f(type_tag<L1>{});
    case PTK_METRIC_LPINF: return f(type_tag<LInf>{});
    case PTK_METRIC_LNINF: return f(type_tag<LNInf>{});
    default: return f(type_tag<L2>{});
  }
}
// float32, the four Euclidean metrics (anything else: L2 squared)
template <class F>
int with_metric(int id, F&& f) {
  return with_euclid_of<ptk::MetricL2, ptk::MetricL1, ptk::MetricLInf, ptk::MetricLNInf>(id, std::forward<F>(f));
}
// float32, the two topological metrics (anything else: SE2)
template <class F>
int with_topo(int id, F&& f) {
  return id == PTK_METRIC_SO2 ? f(type_tag<ptk::TopoSO2>{}) : f(type_tag<ptk::TopoSE2>{});
}
// float64, the four Euclidean metrics (anything else: L2 squared)
template <class F>
int with_euclid64(int id, F&& f) {
  return with_euclid_of<ptk::Metric64L2, ptk::Metric64L1, ptk::Metric64LInf, ptk::Metric64LNInf>(id, std::forward<F>(f));
}
// float64, all six
template <class F>
int with_metric64(int id, F&& f) {
  if (id == PTK_METRIC_SO2) return f(type_tag<ptk::Topo64SO2>{});
  if (id == PTK_METRIC_SE2_SQUARED) return f(type_tag<ptk::Topo64SE2>{});
  return with_euclid64(id, std::forward<F>(f));
}

}  // namespace ptkd
