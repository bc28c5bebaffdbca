// kmpc_solve_bigbox.hip — the box form of the large-window solve kernel (kmpc_solve_big.h, BOX: the
// per-asset position limit w <= a.max_weight, kmpc_solve_box_ws): HM = 10 (H <= 10) and HM = 21
// (H <= 21), each at 256 / 512 / 1024 threads, the runtime constraint case alone. Built at the
// options of kmpc_solve_big.hip.
#include "kmpc_solve_big.h"

namespace kmpc {

size_t big_box_ws_bytes(const SolveArgs& a) {
    return a.H <= 10 ? big::ws_bytes<10, true>(a) : big::ws_bytes<21, true>(a);
}

int big_box_launch(const SolveArgs& a, void* ws, size_t ws_size, hipStream_t stream) {
    return a.H <= 10 ? big::launch<10, true>(a, ws, ws_size, stream) : big::launch<21, true>(a, ws, ws_size, stream);
}

}  // namespace kmpc
