// Discrete plugins: the reverse-sweep kernel of csrc/mi_ode_discrete_row.h for a generated row-local f and its vjp, compiled into their
// own shared object (tfdiffeq_amd.lower.discrete_source writes the translation unit):
//
//   #include "mi_ode_discrete_plugin.h"
//   namespace mi { template <typename T> struct RhsUser {
//     static constexpr int D = 2, P = 4; ...
//     operator()(T t, const T* y, T* k) const;                                   // f
//     template <class ACC> void vjp(T t, const T* y, const T* kbar, T* ybar, ACC& acc) const;   // ybar = (df/dy)^T kbar, acc.add(i, (df/dtheta_i)^T kbar)
//   }; }
//   MI_ODE_DEFINE_DISCRETE_PLUGIN(mi::RhsUser)
//
// mi_ode_discrete_plugin_get(dtype) returns the table that goes into mi_ode_rhs.plugin of a mi_ode_discrete_row_sweep call.  The header
// does not include mi_ode_plugin.h: a change here leaves the cache of compiled row-local plugins alone.
#pragma once
#include "mi_ode_discrete_row.h"

namespace mi {
template <typename T, class RHS>
struct DiscretePlugin {
  static const mi_ode_discrete_row_plugin* table(int dtype) {
    static const mi_ode_discrete_row_plugin t = {MI_ODE_DISCRETE_PLUGIN_ABI, dtype, RHS::D, RHS::P, &DiscreteRowLaunch<T, RHS>::sweep};
    return &t;
  }
};
}  // namespace mi

#if !defined(MI_ODE_PLUGIN_F32) && !defined(MI_ODE_PLUGIN_F64)
#define MI_ODE_PLUGIN_F32 1
#define MI_ODE_PLUGIN_F64 1
#endif
#ifdef MI_ODE_PLUGIN_F64
#define MI_ODE_DISCRETE_CASE_F64(RHS) if (dtype == MI_ODE_F64) return mi::DiscretePlugin<double, RHS<double>>::table(MI_ODE_F64);
#else
#define MI_ODE_DISCRETE_CASE_F64(RHS)
#endif
#ifdef MI_ODE_PLUGIN_F32
#define MI_ODE_DISCRETE_CASE_F32(RHS) if (dtype == MI_ODE_F32) return mi::DiscretePlugin<float, RHS<float>>::table(MI_ODE_F32);
#else
#define MI_ODE_DISCRETE_CASE_F32(RHS)
#endif

#define MI_ODE_DEFINE_DISCRETE_PLUGIN(RHS)                                               \
  extern "C" const mi_ode_discrete_row_plugin* mi_ode_discrete_plugin_get(int dtype) {   \
    MI_ODE_DISCRETE_CASE_F64(RHS)                                                        \
    MI_ODE_DISCRETE_CASE_F32(RHS)                                                        \
    return nullptr;                                                                      \
  }
