// TEST INFRASTRUCTURE ONLY -- mixed_sweep.cpp's method (a stand-alone host program over the emulator build of the kernel
// sources, every library-sized buffer EXACTLY its declared size inside a poisoned heap block, every byte 0xFF at the start;
// built with -fsanitize=alignment,address by tools/workspace_sweep.sh) for the R-GCN model's mixed launch:
//   rgcn_mixed_sweep case off
//     case  rgcn_mixed    mpqe_rgcn_mixed_desc_build + mpqe_rgcn_fwd_mixed + mpqe_rgcn_embed_mixed with the descriptor block and
//                         the workspace, a chain and an intersection query type, every readout
//     off   0: buffers 256-byte aligned; 4: 4 bytes past a 256-byte boundary -- the call may then refuse
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <sanitizer/asan_interface.h>

#include "mpqe_amd.h"

namespace {
int g_off = 0;
unsigned g_rng = 4711u;
float rnd() {       // (-0.5, 0.5)
    g_rng = g_rng * 1664525u + 1013904223u;
    return (float)(g_rng >> 8) / 16777216.f - 0.5f;
}
void *exact(size_t n) {
    const size_t total = n + 1024;
    char *raw = static_cast<char *>(malloc(total));
    char *p = raw + 256;
    p += (256 - reinterpret_cast<uintptr_t>(p) % 256) % 256 + g_off;
    memset(raw, 0xFF, total);
    ASAN_POISON_MEMORY_REGION(raw, p - raw);
    ASAN_POISON_MEMORY_REGION(p + n, raw + total - (p + n));
    return p;
}
// n floats of (-0.5, 0.5) in a block of their own, 16-byte aligned (what the library asks of tables and matrices)
float *floats16(size_t n) {
    float *p = static_cast<float *>(aligned_alloc(16, (n * 4 + 15) / 16 * 16));
    for (size_t i = 0; i < n; ++i) p[i] = rnd();
    return p;
}
int verdict(const std::string &what, int st, bool ok) {
    const bool refused = g_off && (st == MPQE_ERR_INVALID_ARG || st == MPQE_ERR_WORKSPACE || st == MPQE_ERR_UNSUPPORTED);
    if (refused) {
        printf("%s: refused (%d)\n", what.c_str(), st);
        return 0;
    }
    if (st != MPQE_OK || !ok) {
        printf("%s: status %d, outputs %s\n", what.c_str(), st, ok ? "as expected" : "NOT as expected");
        return 1;
    }
    printf("%s: ok\n", what.c_str());
    return 0;
}

int rgcn_mixed_case(int query_type, int readout, int64_t D) {
    const int64_t rows = 24, F = 4, Q = 131, R = 5, modes = 3;
    const int passes = 2;
    mpqe_template_t info;
    if (mpqe_template_info(query_type, &info) != MPQE_OK) return 1;
    const int A = info.num_anchors;
    const float *tables[2] = {floats16(rows * D), floats16(rows * D)};
    const int64_t table_rows[2] = {rows, rows};
    const float *mode_emb = floats16(modes * D);
    const float *basis[2] = {floats16(R * D * D), floats16(R * D * D)}, *root[2] = {floats16(D * D), floats16(D * D)};
    const float *bias[2] = {floats16(D), nullptr};
    std::vector<int32_t> recs(F * MPQE_RGCN_MIX_REC_INTS, 0);
    for (int f = 0; f < F; ++f) {
        int32_t *r = recs.data() + f * MPQE_RGCN_MIX_REC_INTS;
        for (int e = 0; e < 3; ++e) r[e] = (f + 2 * e) % R;
        for (int a = 0; a < 3; ++a) r[3 + a] = (f + a) % 2;
        for (int v = 0; v < 3; ++v) r[6 + v] = (f + v) % modes;
        r[9] = f % 2;
    }
    // runs of 1, 63, 64 and 3 queries: stretches that end inside, at and past a block of 64
    std::vector<int64_t> fo(Q), neg_off(Q + 1, 0), anchors(Q * A);
    for (int64_t q = 0; q < Q; ++q) {
        fo[q] = q < 1 ? 0 : q < 64 ? 1 : q < 128 ? 2 : 3;
        neg_off[q + 1] = neg_off[q] + (q * 7) % 19;
        for (int a = 0; a < A; ++a) anchors[q * A + a] = (q * 3 + 11 * a) % rows;
    }
    const int64_t n = Q + neg_off[Q];
    std::vector<int64_t> ids(n), qrow(n);
    for (int64_t q = 0; q < Q; ++q) {
        ids[q] = (q * 5) % rows;
        qrow[q] = q;
        for (int64_t j = neg_off[q]; j < neg_off[q + 1]; ++j) {
            ids[Q + j] = (j * 13) % rows;
            qrow[Q + j] = q;
        }
    }
    std::vector<float> scores(n, NAN), q_out(Q * D, NAN);
    int32_t err = 0;
    const std::string what = std::string("rgcn_mixed (type ") + std::to_string(query_type) + ", readout " +
                             std::to_string(readout) + ", D " + std::to_string(D) + ")";
    const size_t need = mpqe_rgcn_mixed_desc_bytes(F);
    void *desc = exact(need);
    int st = mpqe_rgcn_mixed_desc_build(query_type, recs.data(), F, tables, table_rows, 2, modes, desc, need, nullptr);
    if (st != MPQE_OK) return verdict(what + ": descriptors", st, true);
    const size_t wneed = mpqe_rgcn_mixed_workspace_bytes(query_type, Q, D);
    void *ws = exact(wneed);
    st = mpqe_rgcn_fwd_mixed(query_type, F, desc, need, nullptr, 0, mode_emb, basis, root, bias, R, passes, readout, D, fo.data(),
                             anchors.data(), Q, ids.data(), qrow.data(), n, 1e-8f, ws, wneed, scores.data(), &err, nullptr);
    if (st != MPQE_OK) return verdict(what, st, true);
    bool ok = err == 0;
    for (float x : scores) ok = ok && std::isfinite(x) && std::fabs(x) <= 1.0001f;
    void *ws2 = exact(wneed);
    st = mpqe_rgcn_embed_mixed(query_type, F, desc, need, nullptr, 0, mode_emb, basis, root, bias, R, passes, readout, D, fo.data(),
                               anchors.data(), Q, ws2, wneed, q_out.data(), &err, nullptr);
    ok = ok && err == 0;
    for (float x : q_out) ok = ok && std::isfinite(x);
    return verdict(what, st, ok);
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s case off\n", argv[0]);
        return 2;
    }
    const std::string c = argv[1];
    g_off = atoi(argv[2]);
    if (c == "rgcn_mixed")
        return rgcn_mixed_case(MPQE_Q_2CHAIN, MPQE_READOUT_TM, 48) | rgcn_mixed_case(MPQE_Q_3INTER_CHAIN, MPQE_READOUT_SUM, 16) |
               rgcn_mixed_case(MPQE_Q_3INTER, MPQE_READOUT_MAX, 128);
    fprintf(stderr, "unknown case %s\n", c.c_str());
    return 2;
}
