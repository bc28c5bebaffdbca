// kmpc_solve_hbt10.hip — the path-persistent backtest kernels (kmpc_bt_run.h) of the H = 10
// constant-case ipm_kernel shapes (kmpc_solve_h10_case.hip), built with the same options as that unit.
#include "kmpc_bt_run.h"

namespace kmpc {
template int launch_bt_case<10, false>(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
}  // namespace kmpc
