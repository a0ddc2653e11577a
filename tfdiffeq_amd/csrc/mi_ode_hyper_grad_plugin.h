// Hyper-grad plugins: the gradient kernels of csrc/mi_ode_hyper_grad.h for a generated row-local f and its vjp, compiled into their own
// shared object.  The translation unit is the discrete plugin's (tfdiffeq_amd.lower.discrete_source: operator() + vjp, P = 0) with this
// header and this macro in place of mi_ode_discrete_plugin.h / MI_ODE_DEFINE_DISCRETE_PLUGIN (tfdiffeq_amd.rhs.hyper_grad_source_of):
//
//   #include "mi_ode_hyper_grad_plugin.h"
//   namespace mi { template <typename T> struct RhsUser { static constexpr int D = 3, P = 0; ... operator() ... vjp ... }; }
//   MI_ODE_DEFINE_HYPER_GRAD_PLUGIN(mi::RhsUser)
//
// mi_ode_hyper_grad_plugin_get(dtype) returns the table that goes into mi_ode_rhs.plugin of a mi_ode_hyper_grad descriptor.  The header
// includes mi_ode_hyper.h but no other plugin header: the caches of the forward's hyper plugins stay valid.
#pragma once
#include "mi_ode_hyper_grad.h"
#include "mi_ode_plugin_getter.h"

namespace mi {
template <typename T, class RHS>
struct HyperGradPlugin {
  static const mi_ode_hyper_grad_plugin* table(int dtype) {
    static const mi_ode_hyper_grad_plugin t = {MI_ODE_HYPER_GRAD_PLUGIN_ABI, dtype, RHS::D, &HyperGradLaunch<T, RHS>::run};
    return &t;
  }
};
}  // namespace mi

#define MI_ODE_DEFINE_HYPER_GRAD_PLUGIN(RHS) MI_ODE_DEFINE_PLUGIN_GETTER(mi_ode_hyper_grad_plugin_get, mi_ode_hyper_grad_plugin, mi::HyperGradPlugin, RHS)
