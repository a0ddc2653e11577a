// Rows plugins: the per-trajectory kernel of csrc/mi_ode_rows.h for a user-supplied row-local f (the same functor a row-local plugin
// defines, csrc/mi_ode_plugin.h), compiled into its own shared object - a kind of its own, so that the row-local plugins (and their
// cache) stay as they are and only the systems that ask for per-trajectory step control carry these kernels.  The translation unit is
// the row-local plugin's with this header and this macro in place of mi_ode_plugin.h / MI_ODE_DEFINE_ROWLOCAL_PLUGIN
// (tfdiffeq_amd.rhs.rows_source writes it):
//
//   #include "mi_ode_rows_plugin.h"
//   namespace mi { template <typename T> struct RhsUser { static constexpr int D = 2; ... operator()(T t, const T* y, T* k) ... }; }
//   MI_ODE_DEFINE_ROWS_PLUGIN(mi::RhsUser)
//
// mi_ode_rows_plugin_get(dtype) returns the table mi_ode_integrate_rows takes next to a handle created for the row-local plugin.
#pragma once
#include "mi_ode_host.h"
#include "mi_ode_rows.h"
#include "mi_ode_plugin_getter.h"

namespace mi {
template <typename T, class RHS>
struct RowsPlugin {
  static const mi_ode_rows_plugin* table(int dtype) {
    static const mi_ode_rows_plugin t = {MI_ODE_ROWS_PLUGIN_ABI, dtype, RHS::D, 0, &RowsKernels<T, RHS>::fn};
    return &t;
  }
};
}  // namespace mi

#define MI_ODE_DEFINE_ROWS_PLUGIN(RHS) MI_ODE_DEFINE_PLUGIN_GETTER(mi_ode_rows_plugin_get, mi_ode_rows_plugin, mi::RowsPlugin, RHS)
