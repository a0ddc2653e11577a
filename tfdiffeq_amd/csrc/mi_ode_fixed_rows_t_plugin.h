// Fixed-rows-t plugins: the fixed-grid kernel with per-row times and lengths (csrc/mi_ode_fixed_rows_t.h) for a user-supplied row-local
// f - the functor a row-local plugin defines (csrc/mi_ode_plugin.h), compiled into a shared object of its own, as the rows-t plugin
// (csrc/mi_ode_rows_t_plugin.h) is: only the systems that are solved on a fixed grid with a 2-D `t` carry this kernel, and the row-local
// plugins (and their cache) stay as they are.  The translation unit is the row-local plugin's with this header and this macro in place
// of mi_ode_plugin.h / MI_ODE_DEFINE_ROWLOCAL_PLUGIN (tfdiffeq_amd.rhs.fixed_rows_t_source_of writes it):
//
//   #include "mi_ode_fixed_rows_t_plugin.h"
//   namespace mi { template <typename T> struct RhsUser { static constexpr int D = 2; ... operator()(T t, const T* y, T* k) ... }; }
//   MI_ODE_DEFINE_FIXED_ROWS_T_PLUGIN(mi::RhsUser)
//
// mi_ode_fixed_rows_t_plugin_get(dtype) returns the table mi_ode_integrate_fixed_rows_t takes next to a handle created for the row-local
// plugin.
#pragma once
#include "mi_ode_host.h"
#include "mi_ode_fixed_rows_t.h"

namespace mi {
template <typename T, class RHS>
struct FixedRowsTPlugin {
  static const mi_ode_fixed_rows_t_plugin* table(int dtype) {
    static const mi_ode_fixed_rows_t_plugin t = {MI_ODE_FIXED_ROWS_T_PLUGIN_ABI, dtype, RHS::D, 0, (const void*)k_fixed_rowlocal_t<T, RHS>};
    return &t;
  }
};
}  // namespace mi

#if !defined(MI_ODE_PLUGIN_F32) && !defined(MI_ODE_PLUGIN_F64)
#define MI_ODE_PLUGIN_F32 1
#define MI_ODE_PLUGIN_F64 1
#endif
#ifdef MI_ODE_PLUGIN_F64
#define MI_ODE_FIXED_ROWS_T_CASE_F64(RHS) if (dtype == MI_ODE_F64) return mi::FixedRowsTPlugin<double, RHS<double>>::table(MI_ODE_F64);
#else
#define MI_ODE_FIXED_ROWS_T_CASE_F64(RHS)
#endif
#ifdef MI_ODE_PLUGIN_F32
#define MI_ODE_FIXED_ROWS_T_CASE_F32(RHS) if (dtype == MI_ODE_F32) return mi::FixedRowsTPlugin<float, RHS<float>>::table(MI_ODE_F32);
#else
#define MI_ODE_FIXED_ROWS_T_CASE_F32(RHS)
#endif

#define MI_ODE_DEFINE_FIXED_ROWS_T_PLUGIN(RHS)                                                       \
  extern "C" const mi_ode_fixed_rows_t_plugin* mi_ode_fixed_rows_t_plugin_get(int dtype) {           \
    MI_ODE_FIXED_ROWS_T_CASE_F64(RHS)                                                                \
    MI_ODE_FIXED_ROWS_T_CASE_F32(RHS)                                                                \
    return nullptr;                                                                                  \
  }
