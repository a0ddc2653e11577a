// The getter every kind of plugin exports: one extern "C" function that maps a state dtype to the kind's table.  A plugin header
// (mi_ode_plugin.h, mi_ode_rows_t_plugin.h, ...) keeps its kernel includes and its factory - a `template <typename T, class RHS> struct`
// with `static const table_type* table(int dtype)` - and defines its macro in one line:
//
//   #define MI_ODE_DEFINE_ROWS_T_PLUGIN(RHS) MI_ODE_DEFINE_PLUGIN_GETTER(mi_ode_rows_t_plugin_get, mi_ode_rows_t_plugin, mi::RowsTPlugin, RHS)
//
// This header includes no kernel header and no plugin header: it is in the #include closure of every kind, so whatever it pulled in would
// tie the caches of all compiled plugins together (tfdiffeq_amd._plugin_build keys a plugin by the headers it sees).
#pragma once
#include "../../include/mi_ode.h"            // MI_ODE_F32 / MI_ODE_F64

// MI_ODE_PLUGIN_F32 / MI_ODE_PLUGIN_F64 select which state dtypes the plugin is built for (both by default)
#if !defined(MI_ODE_PLUGIN_F32) && !defined(MI_ODE_PLUGIN_F64)
#define MI_ODE_PLUGIN_F32 1
#define MI_ODE_PLUGIN_F64 1
#endif
#ifdef MI_ODE_PLUGIN_F64
#define MI_ODE_PLUGIN_GETTER_CASE_F64(Factory, RHS) if (dtype == MI_ODE_F64) return Factory<double, RHS<double>>::table(MI_ODE_F64);
#else
#define MI_ODE_PLUGIN_GETTER_CASE_F64(Factory, RHS)
#endif
#ifdef MI_ODE_PLUGIN_F32
#define MI_ODE_PLUGIN_GETTER_CASE_F32(Factory, RHS) if (dtype == MI_ODE_F32) return Factory<float, RHS<float>>::table(MI_ODE_F32);
#else
#define MI_ODE_PLUGIN_GETTER_CASE_F32(Factory, RHS)
#endif

#define MI_ODE_DEFINE_PLUGIN_GETTER(getter_symbol, table_type, Factory, RHS)             \
  extern "C" const table_type* getter_symbol(int dtype) {                                \
    MI_ODE_PLUGIN_GETTER_CASE_F64(Factory, RHS)                                          \
    MI_ODE_PLUGIN_GETTER_CASE_F32(Factory, RHS)                                          \
    return nullptr;                                                                      \
  }
