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
#include "mi_ode_plugin_getter.h"

namespace mi {
template <typename T, class RHS>
struct HyperPlugin {
  static const mi_ode_hyper_plugin* table(int dtype) {
    static const mi_ode_hyper_plugin t = {MI_ODE_HYPER_PLUGIN_ABI, dtype, RHS::D, &HyperLaunch<T, RHS>::traj, &HyperLaunch<T, RHS>::resid};
    return &t;
  }
};
}  // namespace mi

#define MI_ODE_DEFINE_HYPER_PLUGIN(RHS) MI_ODE_DEFINE_PLUGIN_GETTER(mi_ode_hyper_plugin_get, mi_ode_hyper_plugin, mi::HyperPlugin, RHS)
