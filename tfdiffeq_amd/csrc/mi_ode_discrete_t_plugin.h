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

namespace mi {
template <typename T, class RHS>
struct DiscreteTPlugin {
  static const mi_ode_discrete_row_t_plugin* table(int dtype) {
    static const mi_ode_discrete_row_t_plugin t = {MI_ODE_DISCRETE_T_PLUGIN_ABI, dtype, RHS::D, RHS::P, &DiscreteRowTLaunch<T, RHS>::sweep};
    return &t;
  }
};
}  // namespace mi

#if !defined(MI_ODE_PLUGIN_F32) && !defined(MI_ODE_PLUGIN_F64)
#define MI_ODE_PLUGIN_F32 1
#define MI_ODE_PLUGIN_F64 1
#endif
#ifdef MI_ODE_PLUGIN_F64
#define MI_ODE_DISCRETE_T_CASE_F64(RHS) if (dtype == MI_ODE_F64) return mi::DiscreteTPlugin<double, RHS<double>>::table(MI_ODE_F64);
#else
#define MI_ODE_DISCRETE_T_CASE_F64(RHS)
#endif
#ifdef MI_ODE_PLUGIN_F32
#define MI_ODE_DISCRETE_T_CASE_F32(RHS) if (dtype == MI_ODE_F32) return mi::DiscreteTPlugin<float, RHS<float>>::table(MI_ODE_F32);
#else
#define MI_ODE_DISCRETE_T_CASE_F32(RHS)
#endif

#define MI_ODE_DEFINE_DISCRETE_T_PLUGIN(RHS)                                                 \
  extern "C" const mi_ode_discrete_row_t_plugin* mi_ode_discrete_t_plugin_get(int dtype) {   \
    MI_ODE_DISCRETE_T_CASE_F64(RHS)                                                          \
    MI_ODE_DISCRETE_T_CASE_F32(RHS)                                                          \
    return nullptr;                                                                          \
  }
