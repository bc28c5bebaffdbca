// kmpc_solve_psw10.hip — the sweep form of the path-persistent backtest kernels (kmpc_bt_run.h) of
// the packed shapes with H = 10, built with the same options as kmpc_solve_p10.hip.
#include "kmpc_solve_kernel.h"
#include "kmpc_bt_run.h"

namespace kmpc {
template int launch_bt_packed<10, true>(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
}  // namespace kmpc
