// kmpc_solve_hswbox5.hip — the sweep form of the path-persistent backtest kernels (kmpc_bt_run.h) of
// the box-case shapes for H <= 5, built with the same options as kmpc_solve_hbtbox5.hip.
#include "kmpc_bt_run.h"

namespace kmpc {
template int launch_bt_box<5, true>(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
}  // namespace kmpc
