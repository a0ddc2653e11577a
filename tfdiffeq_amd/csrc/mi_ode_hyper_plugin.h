// Hyper plugins: the hypersolver kernels of csrc/mi_ode_hyper.h for a user-supplied row-local f (the same functor a row-local plugin
// defines, csrc/mi_ode_plugin.h), compiled into their own shared object.  The translation unit is the row-local plugin's with this
// header and this macro in place of mi_ode_plugin.h / MI_ODE_DEFINE_ROWLOCAL_PLUGIN (tfdiffeq_amd.rhs.CustomRowLocal.hyper_source
// writes it):
//
//   #include "mi_ode_hyper_plugin.h"
//   namespace mi { template <typename T> struct RhsUser { static constexpr int D = 2; ... operator()(T t, const T* y, T* k) ... }; }
//   MI_ODE_DEFINE_HYPER_PLUGIN(mi::RhsUser)
//
// mi_ode_hyper_plugin_get(dtype) returns the table that goes into mi_ode_rhs.plugin of a mi_ode_hyper descriptor.
#pragma once
#include "mi_ode_hyper.h"

namespace mi {
template <typename T, class RHS>
struct HyperPlugin {
  static const mi_ode_hyper_plugin* table(int dtype) {
    static const mi_ode_hyper_plugin t = {MI_ODE_HYPER_PLUGIN_ABI, dtype, RHS::D, &HyperLaunch<T, RHS>::traj, &HyperLaunch<T, RHS>::resid};
    return &t;
  }
};
}  // namespace mi

#if !defined(MI_ODE_PLUGIN_F32) && !defined(MI_ODE_PLUGIN_F64)
#define MI_ODE_PLUGIN_F32 1
#define MI_ODE_PLUGIN_F64 1
#endif
#ifdef MI_ODE_PLUGIN_F64
#define MI_ODE_HYPER_CASE_F64(RHS) if (dtype == MI_ODE_F64) return mi::HyperPlugin<double, RHS<double>>::table(MI_ODE_F64);
#else
#define MI_ODE_HYPER_CASE_F64(RHS)
#endif
#ifdef MI_ODE_PLUGIN_F32
#define MI_ODE_HYPER_CASE_F32(RHS) if (dtype == MI_ODE_F32) return mi::HyperPlugin<float, RHS<float>>::table(MI_ODE_F32);
#else
#define MI_ODE_HYPER_CASE_F32(RHS)
#endif

#define MI_ODE_DEFINE_HYPER_PLUGIN(RHS)                                                  \
  extern "C" const mi_ode_hyper_plugin* mi_ode_hyper_plugin_get(int dtype) {             \
    MI_ODE_HYPER_CASE_F64(RHS)                                                           \
    MI_ODE_HYPER_CASE_F32(RHS)                                                           \
    return nullptr;                                                                      \
  }
