// Rows-t plugins: the per-trajectory kernel with per-row times, lengths and tolerances (csrc/mi_ode_rows_t.h) for a user-supplied
// row-local f - the functor a row-local plugin defines (csrc/mi_ode_plugin.h), compiled into a shared object of its own, beside the rows
// plugin (csrc/mi_ode_rows_plugin.h) and as that one is: only the systems that are solved with a 2-D `t` carry these kernels, and the
// row-local and rows plugins (and their cache) stay as they are.  The translation unit is the row-local plugin's with this header and
// this macro in place of mi_ode_plugin.h / MI_ODE_DEFINE_ROWLOCAL_PLUGIN (tfdiffeq_amd.rhs.rows_t_source_of writes it):
//
//   #include "mi_ode_rows_t_plugin.h"
//   namespace mi { template <typename T> struct RhsUser { static constexpr int D = 2; ... operator()(T t, const T* y, T* k) ... }; }
//   MI_ODE_DEFINE_ROWS_T_PLUGIN(mi::RhsUser)
//
// mi_ode_rows_t_plugin_get(dtype) returns the table mi_ode_integrate_rows_t takes next to a handle created for the row-local plugin.
#pragma once
#include "mi_ode_host.h"
#include "mi_ode_rows_t.h"
#include "mi_ode_plugin_getter.h"

namespace mi {
template <typename T, class RHS>
struct RowsTPlugin {
  static const mi_ode_rows_t_plugin* table(int dtype) {
    static const mi_ode_rows_t_plugin t = {MI_ODE_ROWS_T_PLUGIN_ABI, dtype, RHS::D, 0, &RowsTKernels<T, RHS>::fn};
    return &t;
  }
};
}  // namespace mi

#define MI_ODE_DEFINE_ROWS_T_PLUGIN(RHS) MI_ODE_DEFINE_PLUGIN_GETTER(mi_ode_rows_t_plugin_get, mi_ode_rows_t_plugin, mi::RowsTPlugin, RHS)
