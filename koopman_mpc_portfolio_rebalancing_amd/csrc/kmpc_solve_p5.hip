// kmpc_solve_p5.hip — packed (lane-group) ipm_kernel instantiations for H <= 5 (see
// kmpc_solve_kernel.h, launch_ipm_packed).
#include "kmpc_solve_kernel.h"
#include "kmpc_bt_run.h"

namespace kmpc {
template int launch_ipm_packed<2>(const SolveArgs& a, hipStream_t stream);
template int launch_ipm_packed<5>(const SolveArgs& a, hipStream_t stream);
// the path-persistent backtest kernels of the packed shapes (kmpc_bt_run.h), built with this unit's
// options like the kernels they mirror
template int launch_bt_packed<2, false>(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
template int launch_bt_packed<5, false>(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
}  // namespace kmpc
