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

namespace mi {
template <typename T, class RHS>
struct RowsPlugin {
  static const mi_ode_rows_plugin* table(int dtype) {
    static const mi_ode_rows_plugin t = {MI_ODE_ROWS_PLUGIN_ABI, dtype, RHS::D, 0, &RowsKernels<T, RHS>::fn};
    return &t;
  }
};
}  // namespace mi

#if !defined(MI_ODE_PLUGIN_F32) && !defined(MI_ODE_PLUGIN_F64)
#define MI_ODE_PLUGIN_F32 1
#define MI_ODE_PLUGIN_F64 1
#endif
#ifdef MI_ODE_PLUGIN_F64
#define MI_ODE_ROWS_CASE_F64(RHS) if (dtype == MI_ODE_F64) return mi::RowsPlugin<double, RHS<double>>::table(MI_ODE_F64);
#else
#define MI_ODE_ROWS_CASE_F64(RHS)
#endif
#ifdef MI_ODE_PLUGIN_F32
#define MI_ODE_ROWS_CASE_F32(RHS) if (dtype == MI_ODE_F32) return mi::RowsPlugin<float, RHS<float>>::table(MI_ODE_F32);
#else
#define MI_ODE_ROWS_CASE_F32(RHS)
#endif

#define MI_ODE_DEFINE_ROWS_PLUGIN(RHS)                                                   \
  extern "C" const mi_ode_rows_plugin* mi_ode_rows_plugin_get(int dtype) {               \
    MI_ODE_ROWS_CASE_F64(RHS)                                                            \
    MI_ODE_ROWS_CASE_F32(RHS)                                                            \
    return nullptr;                                                                      \
  }
