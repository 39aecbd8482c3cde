// The transposed aggregation of the INPUT-ONLY backward (layer.hip layer_backward_impl(input_only), eagcn_model_backward_input): the
// instantiations of lagg_kernel with EDGE = false -- no P rows of the edge gradients, no row dots, no bond-type histogram, no flush
// into the accumulator slabs -- and the Concate eval form that re-forms dH from the upstream gradient and the row mask (CROWS).  Kept
// apart from lagg.hip, whose five instantiations (forward and edge-gradient forms) are what tests/test_isa_cpu.py pins.  Everything
// the input-only forms add to the shared template is guarded at compile time (EDGE / CROWS) and AggArgs.w_rowm sits in padding, so
// those five compile to the same instructions as before the input-only forms existed.
// Same grid, same policy as the edge forms (launch_lagg_bwd computes the grid and hands it here).
#include "lagg_kernel.h"

namespace eagcn {

int launch_lagg_bwd_input(const AggArgs& a, const EdgeArgs& e, dim3 grid, hipStream_t s) {
    if (a.w_rowm) lagg_kernel<true, true, true, false, true><<<grid, 256, 0, s>>>(a, e);
    else if (a.w_aw) lagg_kernel<true, true, true, false><<<grid, 256, 0, s>>>(a, e);
    else if (a.cpw > 1) lagg_kernel<true, true, false, false><<<grid, 256, 0, s>>>(a, e);
    else lagg_kernel<true, false, false, false><<<grid, 256, 0, s>>>(a, e);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

}  // namespace eagcn
