// tests/send_geom_host/shim.cpp -- TEST INFRASTRUCTURE ONLY: the datagram / frame send's choice of
// kernels and launch geometry (send_form of quicknet_amd/csrc/qfec_geom.hpp) behind a C interface,
// for tests/test_tx_model.py.  Never shipped.
#include "../../quicknet_amd/csrc/qfec_geom.hpp"

extern "C" {
// returns the SendKind; out = {line, gpw, ts, tn, lpg, rec_words}, *per = groups per launch (pair)
int send_form(int instance, int n, int checksum, long long pitch, long long row_pitch, int prefix, unsigned* out,
              long long* per) {
    const qfec::SendForm f = qfec::send_form(instance != 0, n, checksum, (uint64_t)pitch, (uint64_t)row_pitch, prefix);
    out[0] = f.line;
    out[1] = f.gpw;
    out[2] = f.ts;
    out[3] = f.tn;
    out[4] = f.lpg;
    out[5] = f.rec_words;
    *per = (long long)f.per;
    return f.kind;
}
// u32 words the body leaves in d_shards for a batch of `groups`
unsigned long long send_part_words(int n, int checksum, long long pitch, long long row_pitch, unsigned long long groups) {
    return qfec::send_part_words(qfec::send_form(true, n, checksum, (uint64_t)pitch, (uint64_t)row_pitch, 0), groups);
}
// how many launches for_group_chunks makes, and the most groups in one of them; -1 unless they
// cover [0, groups) in order, each starting on a multiple of `align`
long long send_chunks(long long groups, long long per, long long align, long long* most) {
    long long n = 0, at = 0;
    *most = 0;
    qfec::for_group_chunks(groups, per, [&](long long g0, long long gn) {
        if (g0 != at || gn < 1 || g0 % align) return -1;
        at += gn;
        if (gn > *most) *most = gn;
        ++n;
        return 0;
    });
    return at == groups ? n : -1;
}
}
