// kmpc_solve_hsw10.hip — the sweep form of the path-persistent backtest kernels (kmpc_bt_run.h) of
// the H = 10 constant-case shapes, built with the same options as kmpc_solve_hbt10.hip.
#include "kmpc_bt_run.h"

namespace kmpc {
template int launch_bt_case<10, true>(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
}  // namespace kmpc
