// TEST INFRASTRUCTURE ONLY -- mixed_sweep.cpp's method (a stand-alone host program over the emulator build of the kernel
// sources, every library-sized buffer EXACTLY its declared size inside a poisoned heap block, every byte 0xFF at the start;
// built with -fsanitize=alignment,address by tools/workspace_sweep.sh) for the R-GCN model's mixed TRAINING calls:
//   rgcn_mixed_train_sweep case off
//     case  rgcn_mixed_train  mpqe_rgcn_mixed_desc_build + mpqe_rgcn_mixed_index_build + mpqe_rgcn_fwd_mixed_save +
//                             mpqe_rgcn_bwd_mixed (through grad_scores, then through grad_q) with the two blocks and the
//                             workspace, a chain and two intersection query types, every readout
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

float *zeros16(size_t n) {
    float *p = floats16(n);
    for (size_t i = 0; i < n; ++i) p[i] = 0.f;
    return p;
}

int train_case(int query_type, int readout, int64_t D) {
    const int64_t rows = 24, F = 4, Q = 131, R = 5, modes = 3;
    const int passes = 3, L = 2, T = 2;
    mpqe_template_t info;
    if (mpqe_template_info(query_type, &info) != MPQE_OK) return 1;
    const int A = info.num_anchors;
    const float *tables[2] = {floats16(rows * D), floats16(rows * D)};
    const int64_t table_rows[2] = {rows, rows};
    const float *mode_emb = floats16(modes * D);
    const float *lb[2] = {floats16(R * D * D), floats16(R * D * D)}, *lr[2] = {floats16(D * D), floats16(D * D)};
    const float *lbias[2] = {floats16(D), nullptr};
    const int lop[3] = {0, 1, 1};
    const float *basis[3], *root[3], *bias[3];
    for (int p = 0; p < passes; ++p) {
        basis[p] = lb[lop[p]];
        root[p] = lr[lop[p]];
        bias[p] = lbias[lop[p]];
    }
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
        neg_off[q + 1] = neg_off[q] + (q * 7) % 5;
        for (int a = 0; a < A; ++a) anchors[q * A + a] = (q * 3 + 11 * a) % rows;
    }
    const int64_t n = Q + neg_off[Q];
    std::vector<int64_t> ids(n);
    for (int64_t q = 0; q < Q; ++q) {
        ids[q] = (q * 5) % rows;
        for (int64_t j = neg_off[q]; j < neg_off[q + 1]; ++j) ids[Q + j] = (j * 13) % rows;
    }
    std::vector<float> scores(n, NAN), gs(n), gq(Q * D);
    for (float &x : gs) x = rnd();
    for (float &x : gq) x = rnd();
    float *q_out = zeros16(Q * D);
    float *gt[2] = {zeros16(rows * D), zeros16(rows * D)}, *gme = zeros16(modes * D);
    float *gb[2] = {zeros16(R * D * D), zeros16(R * D * D)}, *gr[2] = {zeros16(D * D), zeros16(D * D)};
    float *gbias[2] = {zeros16(D), nullptr};
    int32_t err = 0;
    const std::string what = std::string("rgcn_mixed_train (type ") + std::to_string(query_type) + ", readout " +
                             std::to_string(readout) + ", D " + std::to_string(D) + ")";
    const size_t need = mpqe_rgcn_mixed_desc_bytes(F), ineed = mpqe_rgcn_mixed_index_bytes(F);
    void *desc = exact(need), *index = exact(ineed);
    int st = mpqe_rgcn_mixed_desc_build(query_type, recs.data(), F, tables, table_rows, T, modes, desc, need, nullptr);
    if (st != MPQE_OK) return verdict(what + ": descriptors", st, true);
    st = mpqe_rgcn_mixed_index_build(query_type, recs.data(), F, index, ineed, nullptr);
    if (st != MPQE_OK) return verdict(what + ": index", st, true);
    bool ok = true;
    for (int pass = 0; pass < 2; ++pass) {
        // pass 0: scored pairs, the backward through grad_scores; pass 1: no pairs, the backward through grad_q
        const int64_t np = pass == 0 ? n : 0;
        const size_t wneed = mpqe_rgcn_mixed_train_workspace_bytes(query_type, Q, np, D, passes, R, T, modes, L);
        if (wneed == 0) return verdict(what + ": workspace size", MPQE_ERR_UNSUPPORTED, false);
        void *ws = exact(wneed);
        st = mpqe_rgcn_fwd_mixed_save(query_type, F, desc, need, nullptr, 0, mode_emb, basis, root, bias, R, passes, readout, D,
                                      fo.data(), anchors.data(), Q, ids.data(), neg_off.data(), np, 1e-8f, T, modes, L, ws, wneed,
                                      scores.data(), q_out, &err, nullptr);
        if (st != MPQE_OK) return verdict(what + ": save", st, true);
        st = mpqe_rgcn_bwd_mixed(query_type, F, desc, need, index, ineed, nullptr, 0, mode_emb, basis, root, bias, R, passes,
                                 readout, D, fo.data(), anchors.data(), Q, ids.data(), neg_off.data(), np, 1e-8f, T, modes, L, lop,
                                 pass == 0 ? gs.data() : nullptr, pass == 0 ? nullptr : gq.data(), gt, gme, gb, gr, gbias, ws,
                                 wneed, &err, nullptr);
        if (st != MPQE_OK) return verdict(what + ": backward", st, true);
    }
    ok = ok && err == 0;
    for (float x : scores) ok = ok && std::isfinite(x) && std::fabs(x) <= 1.0001f;
    bool any = false;
    for (int64_t i = 0; i < Q * D; ++i) ok = ok && std::isfinite(q_out[i]);
    for (int t = 0; t < 2; ++t)
        for (int64_t i = 0; i < rows * D; ++i) ok = ok && std::isfinite(gt[t][i]);
    for (int l = 0; l < 2; ++l) {
        for (int64_t i = 0; i < R * D * D; ++i) ok = ok && std::isfinite(gb[l][i]);
        for (int64_t i = 0; i < D * D; ++i) {
            ok = ok && std::isfinite(gr[l][i]);
            any = any || gr[l][i] != 0.f;
        }
    }
    for (int64_t i = 0; i < modes * D; ++i) ok = ok && std::isfinite(gme[i]);
    for (int64_t i = 0; i < D; ++i) ok = ok && std::isfinite(gbias[0][i]);
    return verdict(what, st, ok && any);
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s case off\n", argv[0]);
        return 2;
    }
    const std::string c = argv[1];
    g_off = atoi(argv[2]);
    if (c == "rgcn_mixed_train")
        return train_case(MPQE_Q_2CHAIN, MPQE_READOUT_TM, 48) | train_case(MPQE_Q_3INTER_CHAIN, MPQE_READOUT_SUM, 16) |
               train_case(MPQE_Q_3INTER, MPQE_READOUT_MAX, 128);
    fprintf(stderr, "unknown case %s\n", c.c_str());
    return 2;
}
