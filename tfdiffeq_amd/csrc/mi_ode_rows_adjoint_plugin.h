// Rows-adjoint plugins: the per-trajectory adjoint kernel of csrc/mi_ode_rows_adjoint.h for a generated row-local f and its vjp with
// respect to y, t and the trainable tensors, compiled into their own shared object (tfdiffeq_amd.lower.adjoint_source writes the
// translation unit):
//
//   #include "mi_ode_rows_adjoint_plugin.h"
//   namespace mi { template <typename T> struct RhsUser {
//     static constexpr int D = 3, P = 3; ...
//     operator()(T t, const T* y, T* k) const;                                                  // f
//     template <class ACC> void vjp_t(T t, const T* y, const T* kbar, T* ybar, T& tbar, ACC& acc) const;
//   }; }                     // ybar = (df/dy)^T kbar, tbar = (df/dt)^T kbar, acc.add(i, (df/dtheta_i)^T kbar)
//   MI_ODE_DEFINE_ROWS_ADJOINT_PLUGIN(mi::RhsUser)
//
// mi_ode_rows_adjoint_plugin_get(dtype) returns the table that goes into mi_ode_rhs.plugin of a mi_ode_adjoint_rows call.  A kind of its
// own: the header includes neither mi_ode_plugin.h nor mi_ode_rows_plugin.h, so a change here leaves the caches of compiled row-local
// and rows plugins alone.
#pragma once
#include "mi_ode_host.h"
#include "mi_ode_rows_adjoint.h"
#include "mi_ode_plugin_getter.h"

namespace mi {
template <typename T, class RHS>
struct RowsAdjPlugin {
  static const mi_ode_rows_adjoint_plugin* table(int dtype) {
    static const mi_ode_rows_adjoint_plugin t = {MI_ODE_ROWS_ADJOINT_PLUGIN_ABI, dtype, RHS::D, RHS::P, &RowsAdjLaunch<T, RHS>::launch};
    return &t;
  }
};
}  // namespace mi

#define MI_ODE_DEFINE_ROWS_ADJOINT_PLUGIN(RHS) MI_ODE_DEFINE_PLUGIN_GETTER(mi_ode_rows_adjoint_plugin_get, mi_ode_rows_adjoint_plugin, mi::RowsAdjPlugin, RHS)
