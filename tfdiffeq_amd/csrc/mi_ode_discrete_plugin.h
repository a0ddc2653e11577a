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
#include "mi_ode_plugin_getter.h"

namespace mi {
template <typename T, class RHS>
struct DiscretePlugin {
  static const mi_ode_discrete_row_plugin* table(int dtype) {
    static const mi_ode_discrete_row_plugin t = {MI_ODE_DISCRETE_PLUGIN_ABI, dtype, RHS::D, RHS::P, &DiscreteRowLaunch<T, RHS>::sweep};
    return &t;
  }
};
}  // namespace mi

#define MI_ODE_DEFINE_DISCRETE_PLUGIN(RHS) MI_ODE_DEFINE_PLUGIN_GETTER(mi_ode_discrete_plugin_get, mi_ode_discrete_row_plugin, mi::DiscretePlugin, RHS)
