// tests/update_geom_host/shim.cpp -- TEST INFRASTRUCTURE ONLY: qfec_update's launch geometry
// (wave_geom of quicknet_amd/csrc/qfec_geom.hpp) behind a C interface, for
// tests/test_update_geom_host.py.  Never shipped.
#include "../../quicknet_amd/csrc/qfec_geom.hpp"

extern "C" {
// out = {vec16, cols, wpg}, *per = groups per launch; rows / parity / strides as qfec_update hands them over
void update_geom(unsigned long long rows, unsigned long long parity, int block, long long pitch,
                 unsigned long long rgs, unsigned long long pgs, unsigned* out, long long* per) {
    const qfec::FlatGeom f = qfec::flat_geom((const void*)(uintptr_t)rows, (const void*)(uintptr_t)parity, block, pitch, rgs, pgs);
    const qfec::WaveGeom w = qfec::wave_geom(f);
    out[0] = f.vec16;
    out[1] = w.cols;
    out[2] = w.wpg;
    *per = w.per;
}
// how many launches for_group_chunks makes, and the most groups in one of them
long long update_chunks(long long groups, long long per, long long* most) {
    long long n = 0, at = 0;
    *most = 0;
    qfec::for_group_chunks(groups, per, [&](long long g0, long long gn) {
        if (g0 != at || gn < 1) return -1;
        at += gn;
        if (gn > *most) *most = gn;
        ++n;
        return 0;
    });
    return at == groups ? n : -1;
}
}
