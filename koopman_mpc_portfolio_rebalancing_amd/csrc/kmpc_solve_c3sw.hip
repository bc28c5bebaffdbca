// kmpc_solve_c3sw.hip — the sweep form of the path-persistent backtest kernel (kmpc_bt_run.h) of
// the C3 shape (H = 10, N < 104: 128 threads, the LDL^T arrays in LDS), built with the options of
// kmpc_solve_c3.hip, whose kernel it mirrors.
#ifndef KMPC_SCHUR_BCAST_F64   // as kmpc_solve_c3.hip
#define KMPC_SCHUR_BCAST_F64 1
#endif
#ifndef KMPC_FD_WAIT_ONCE_F64   // the column update's wait states at every chunk, as before: the once-per-step
#define KMPC_FD_WAIT_ONCE_F64 0   // form moved the sibling backtest kernel's allocation and ran behind
#endif
#include "kmpc_solve_kernel.h"
#include "kmpc_bt_run.h"

namespace kmpc {
template int launch_bt_c3<true>(const SolveArgs& a, const BtLaunch& l, hipStream_t stream);
}  // namespace kmpc
