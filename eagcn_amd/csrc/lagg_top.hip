// The transposed aggregation of a Concate TOP layer whose BatchNorm backward takes its column sums from the read-out (layer.hip
// BN2_STAGED_FROM_READOUT): no dH exists in memory, so the staging re-forms it from the rows of the read-out gradient (packed columns,
// as wide as dH), the row mask, the relu test and the dropout draw -- the CROWS staging of the input-only form -- and the edge
// gradients leave from the same gathers as in lagg.hip.  Kept apart from lagg.hip, whose five instantiations tests/test_isa_cpu.py
// pins; tests/test_top_bn_isa_cpu.py holds this one to the same limits (no scratch, three workgroups per CU).
#include "lagg_kernel.h"

namespace eagcn {

int launch_lagg_bwd_top(const AggArgs& a, const EdgeArgs& e, dim3 grid, hipStream_t s) {
    if (a.w_gather) lagg_kernel<true, true, true, true, true, true><<<grid, 256, 0, s>>>(a, e);
    else lagg_kernel<true, true, true, true, true><<<grid, 256, 0, s>>>(a, e);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

}  // namespace eagcn
