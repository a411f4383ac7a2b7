// tests/geom_host/shim.cpp -- TEST INFRASTRUCTURE ONLY: the launch geometry of
// quicknet_amd/csrc/qfec_geom.hpp behind a C interface, for tests/test_geom_host.py.  Never shipped.
#include "../../quicknet_amd/csrc/qfec_geom.hpp"

extern "C" {
// out = {vec16, cols, cols8, wpg8}, per = {flat, 8-byte lanes} groups per launch
void geom_shape(unsigned long long data, unsigned long long parity, int k, int block, long long pitch,
                unsigned long long dgs, unsigned long long pgs, unsigned* out, long long* per) {
    const qfec::FlatGeom f = qfec::flat_geom((const void*)(uintptr_t)data, (const void*)(uintptr_t)parity, block, pitch, dgs, pgs);
    const qfec::Lane8Geom g = qfec::lane8_geom(f, k, block);
    out[0] = f.vec16;
    out[1] = f.cols;
    out[2] = g.cols8;
    out[3] = g.wpg8;
    per[0] = f.per;
    per[1] = g.per;
}
// the chunks for_group_chunks makes, the first `cap` of them into g0 / gn; returns how many there were
long long geom_chunks(long long groups, long long per, long long* g0, long long* gn, long long cap) {
    long long n = 0;
    qfec::for_group_chunks(groups, per, [&](long long a, long long b) {
        if (n < cap) { g0[n] = a; gn[n] = b; }
        ++n;
        return 0;
    });
    return n;
}
// for_group_chunks stops at the first non-zero return and hands it back: the calls made
long long geom_chunks_stop(long long groups, long long per, long long fail_at, int* rc) {
    long long n = 0;
    *rc = qfec::for_group_chunks(groups, per, [&](long long, long long) { return n++ == fail_at ? -7 : 0; });
    return n;
}
}
