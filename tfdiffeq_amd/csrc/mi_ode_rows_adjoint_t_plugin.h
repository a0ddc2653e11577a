// Rows-adjoint-t plugins: the per-trajectory adjoint kernel with per-row times, lengths and tolerances (csrc/mi_ode_rows_adjoint_t.h)
// for a generated row-local f and its vjp - the functor a rows-adjoint plugin defines (csrc/mi_ode_rows_adjoint_plugin.h), compiled into
// a shared object of its own, beside that plugin and as it is: only the modules whose gradients are taken with a 2-D `t` carry this
// kernel, and the rows-adjoint plugins (and their cache) stay as they are.  The translation unit is the rows-adjoint plugin's with this
// header and this macro in place of mi_ode_rows_adjoint_plugin.h / MI_ODE_DEFINE_ROWS_ADJOINT_PLUGIN
// (tfdiffeq_amd.rhs.rows_adjoint_t_source_of writes it):
//
//   #include "mi_ode_rows_adjoint_t_plugin.h"
//   namespace mi { template <typename T> struct RhsUser { static constexpr int D = 3, P = 3; ... operator() ... vjp_t ... }; }
//   MI_ODE_DEFINE_ROWS_ADJOINT_T_PLUGIN(mi::RhsUser)
//
// mi_ode_rows_adjoint_t_plugin_get(dtype) returns the table that goes into mi_ode_rhs.plugin of a mi_ode_adjoint_rows_t call.
#pragma once
#include "mi_ode_host.h"
#include "mi_ode_rows_adjoint_t.h"
#include "mi_ode_plugin_getter.h"

namespace mi {
template <typename T, class RHS>
struct RowsAdjTPlugin {
  static const mi_ode_rows_adjoint_t_plugin* table(int dtype) {
    static const mi_ode_rows_adjoint_t_plugin t = {MI_ODE_ROWS_ADJOINT_T_PLUGIN_ABI, dtype, RHS::D, RHS::P, &RowsAdjTLaunch<T, RHS>::launch};
    return &t;
  }
};
}  // namespace mi

#define MI_ODE_DEFINE_ROWS_ADJOINT_T_PLUGIN(RHS) MI_ODE_DEFINE_PLUGIN_GETTER(mi_ode_rows_adjoint_t_plugin_get, mi_ode_rows_adjoint_t_plugin, mi::RowsAdjTPlugin, RHS)
