// kmpc_solve_psw5.hip — the sweep form of the path-persistent backtest kernels (kmpc_bt_run.h) of
// the packed shapes with H = 2 and H = 5, built with the same options as kmpc_solve_p5.hip.
#include "kmpc_solve_kernel.h"
#include "kmpc_bt_run.h"

namespace kmpc {
template int launch_bt_packed<2, true>(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
template int launch_bt_packed<5, true>(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
}  // namespace kmpc
