// kmpc_solve_hbox5.hip — box-case ipm_kernel instantiations (per-asset position limit,
// kmpc_solve_box) for horizons H <= 5 (see kmpc_solve_kernel.h: launch_ipm_box).
#include "kmpc_solve_kernel.h"

namespace kmpc {
template int launch_ipm_box<5>(const SolveArgs& a, hipStream_t stream);
}  // namespace kmpc
