// float32 instantiations of k_rows_rowlocal_t (mi_ode_rows_t.h) for the trajectory-per-thread catalogue families
#include "mi_ode_host.h"
#include "mi_ode_rows_t.h"

using namespace mi;

const void* mi_rows_t_fn_f32(int family, int S, int ts_dense, int fsal) {
  switch (family) {
    case FAM_CUBIC2: return RowsTKernels<float, RhsCubic2<float>>::fn(S, ts_dense, fsal);
    case FAM_LINEAR2: return RowsTKernels<float, RhsLinear2<float>>::fn(S, ts_dense, fsal);
    case FAM_LV: return RowsTKernels<float, RhsLotkaVolterra<float>>::fn(S, ts_dense, fsal);
    case FAM_LORENZ: return RowsTKernels<float, RhsLorenz<float>>::fn(S, ts_dense, fsal);
    default: return nullptr;
  }
}
