// tests/ptrs_geom_host/shim.cpp -- TEST INFRASTRUCTURE ONLY: the pointer-table calls' launch geometry
// of quicknet_amd/csrc/qfec_geom.hpp behind a C interface, for tests/test_ptrs_host.py.  Never shipped.
#include "../../quicknet_amd/csrc/qfec_geom.hpp"

extern "C" {
// out = {vcols, wpg, tail0, tailn}; returns the groups per launch
long long ptrs_geom_shape(int block, int lane_bytes, unsigned* out) {
    const qfec::PtrsGeom p = qfec::ptrs_geom(block, lane_bytes);
    out[0] = p.vcols;
    out[1] = p.wpg;
    out[2] = p.tail0;
    out[3] = p.tailn;
    return p.per;
}
int ptrs_lanes(int reconstruct, int k) { return qfec::ptrs_lane_bytes(reconstruct != 0, k); }
}
