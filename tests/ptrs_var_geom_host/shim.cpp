// tests/ptrs_var_geom_host/shim.cpp -- TEST INFRASTRUCTURE ONLY: the per-group geometry of the
// pointer-table calls with per-shard lengths (ptrs_var_geom in quicknet_amd/csrc/qfec_geom.hpp, the rule
// the kernels of qfec_ptrs_var.hip apply to every group's own length) behind a C interface, for
// tests/test_ptrs_var_host.py.  Never shipped.
#include "../../quicknet_amd/csrc/qfec_geom.hpp"

extern "C" {
// out = {live, vcols, tail0, tailn} of a group of length len
void ptrs_var_geom_shape(unsigned len, unsigned lane_bytes, unsigned* out) {
    const qfec::PtrsVarGeom v = qfec::ptrs_var_geom(len, lane_bytes);
    out[0] = v.live;
    out[1] = v.vcols;
    out[2] = v.tail0;
    out[3] = v.tailn;
}
// waves per group of the launch, from max_len
unsigned ptrs_var_launch_wpg(int max_len, int lane_bytes) { return qfec::ptrs_geom(max_len, lane_bytes).wpg; }
}
