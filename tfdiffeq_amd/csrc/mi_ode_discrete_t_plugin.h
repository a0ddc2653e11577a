// Discrete-t plugins: the reverse-sweep kernel with per-row times and lengths (csrc/mi_ode_discrete_row_t.h) for a generated row-local f
// and its vjp, compiled into a shared object of its own, beside the discrete plugin (csrc/mi_ode_discrete_plugin.h): only the systems
// differentiated over a 2-D `t` carry this kernel, and the discrete plugins (and their cache) stay as they are.  The translation unit
// is the discrete plugin's (tfdiffeq_amd.lower.discrete_source) with this header and this macro in place of mi_ode_discrete_plugin.h /
// MI_ODE_DEFINE_DISCRETE_PLUGIN (tfdiffeq_amd.rhs.discrete_t_source_of writes it):
//
//   #include "mi_ode_discrete_t_plugin.h"
//   namespace mi { template <typename T> struct RhsUser { static constexpr int D = 2, P = 4; ... operator() ... vjp ... }; }
//   MI_ODE_DEFINE_DISCRETE_T_PLUGIN(mi::RhsUser)
//
// mi_ode_discrete_t_plugin_get(dtype) returns the table that goes into mi_ode_rhs.plugin of a mi_ode_discrete_row_sweep_t call.
#pragma once
#include "mi_ode_discrete_row_t.h"
#include "mi_ode_plugin_getter.h"

namespace mi {
template <typename T, class RHS>
struct DiscreteTPlugin {
  static const mi_ode_discrete_row_t_plugin* table(int dtype) {
    static const mi_ode_discrete_row_t_plugin t = {MI_ODE_DISCRETE_T_PLUGIN_ABI, dtype, RHS::D, RHS::P, &DiscreteRowTLaunch<T, RHS>::sweep};
    return &t;
  }
};
}  // namespace mi

#define MI_ODE_DEFINE_DISCRETE_T_PLUGIN(RHS) MI_ODE_DEFINE_PLUGIN_GETTER(mi_ode_discrete_t_plugin_get, mi_ode_discrete_row_t_plugin, mi::DiscreteTPlugin, RHS)
