// float32 instantiations of k_fixed_rowlocal_t (mi_ode_fixed_rows_t.h) for the trajectory-per-thread catalogue families
#include "mi_ode_host.h"
#include "mi_ode_fixed_rows_t.h"

using namespace mi;

const void* mi_fixed_rows_t_fn_f32(int family) {
  switch (family) {
    case FAM_CUBIC2: return (const void*)k_fixed_rowlocal_t<float, RhsCubic2<float>>;
    case FAM_LINEAR2: return (const void*)k_fixed_rowlocal_t<float, RhsLinear2<float>>;
    case FAM_LV: return (const void*)k_fixed_rowlocal_t<float, RhsLotkaVolterra<float>>;
    case FAM_LORENZ: return (const void*)k_fixed_rowlocal_t<float, RhsLorenz<float>>;
    default: return nullptr;
  }
}
