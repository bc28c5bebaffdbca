// kmpc_solve_hsw5.hip — the sweep form of the path-persistent backtest kernels (kmpc_bt_run.h) of
// the H = 5 constant-case shapes, built with the same options as kmpc_solve_hbt5.hip.
#include "kmpc_bt_run.h"

namespace kmpc {
template int launch_bt_case<5, true>(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
}  // namespace kmpc
