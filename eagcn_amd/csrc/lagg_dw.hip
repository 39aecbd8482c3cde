// The transposed aggregation of a FIRST layer (at most 32 input columns) whose input gradient nobody asks for, with the layer's weight
// gradient formed in its epilogue (lagg_kernel.h DWF; layer.hip plan_layer's fused first-layer route): dP -- T x Fp floats with no reader
// but the product dWcat = X^T.dP -- is neither stored nor read back, and that product is no launch of its own.  Kept apart from
// lagg.hip, whose five instantiations tests/test_isa_cpu.py pins; tests/test_first_layer_fused_cpu.py holds these two to the same
// limits (no scratch, at most 168 registers, three workgroups' LDS per CU).
#include "lagg_kernel.h"

namespace eagcn {

int launch_lagg_bwd_dw(const AggArgs& a, const EdgeArgs& e, dim3 grid, hipStream_t s) {
    EAGCN_CHECK_ARG(a.fx && a.dw && a.fx_ld >= 1 && a.fx_ld <= LG_CW && a.dw_ny >= 1 && (int)grid.y == a.dw_ny && !a.planes.p && !a.w_aw,
                    "lagg: the weight-gradient epilogue takes at most 32 input columns and one slab per workgroup row");
    if (a.cpw > 1) lagg_kernel<true, true, false, true, false, false, true><<<grid, 256, 0, s>>>(a, e);
    else lagg_kernel<true, false, false, true, false, false, true><<<grid, 256, 0, s>>>(a, e);
    EAGCN_LAUNCH_CHECK();
    return EAGCN_OK;
}

}  // namespace eagcn
