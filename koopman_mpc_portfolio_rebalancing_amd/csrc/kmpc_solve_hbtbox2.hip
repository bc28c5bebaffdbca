// kmpc_solve_hbtbox2.hip — the path-persistent backtest kernels (kmpc_bt_run.h) of the box-case
// ipm_kernel shapes for H <= 2 (kmpc_solve_hbox2.hip: per-asset position limit), built with the same
// options as that unit.
#include "kmpc_bt_run.h"

namespace kmpc {
template int launch_bt_box<2, false>(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
}  // namespace kmpc
