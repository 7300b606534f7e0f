// TEST INFRASTRUCTURE ONLY -- workspace_sweep.cpp's method (a stand-alone host program over the emulator build of the kernel
// sources, every library-sized buffer EXACTLY its declared size inside a poisoned heap block, every byte 0xFF at the start;
// built with -fsanitize=alignment,address by tools/workspace_sweep.sh) for the entry points that work on queries of
// different formulas at once:
//   mixed_sweep case off
//     case  auc_segments  mpqe_eval_auc_segments with its workspace
//           gqe_mixed     mpqe_gqe_mixed_desc_build + mpqe_gqe_fwd_mixed with the descriptor block, both forms
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
int verdict(const char *what, int st, bool ok) {
    const bool refused = g_off && (st == MPQE_ERR_INVALID_ARG || st == MPQE_ERR_WORKSPACE);
    if (refused) {
        printf("%s: refused (%d)\n", what, st);
        return 0;
    }
    if (st != MPQE_OK || !ok) {
        printf("%s: status %d, outputs %s\n", what, st, ok ? "as expected" : "NOT as expected");
        return 1;
    }
    printf("%s: ok\n", what);
    return 0;
}

int auc_segments_case() {
    const int64_t lens_p[5] = {3, 0, 70, 2100, 1}, lens_n[5] = {2100, 5, 0, 65, 1};
    std::vector<int64_t> po(6, 0), no(6, 0);
    for (int s = 0; s < 5; ++s) {
        po[s + 1] = po[s] + lens_p[s];
        no[s + 1] = no[s] + lens_n[s];
    }
    std::vector<float> pos(po[5]), neg(no[5]);
    for (auto &x : pos) x = std::floor(8.f * rnd());        // few distinct values: ties
    for (auto &x : neg) x = std::floor(8.f * rnd());
    std::vector<uint64_t> u2(5, 77);
    const size_t need = mpqe_eval_auc_segments_workspace_bytes(po[5], no[5], 5);
    void *ws = exact(need);
    const int st = mpqe_eval_auc_segments(pos.data(), po[5], neg.data(), no[5], po.data(), no.data(), 5, u2.data(), ws, need,
                                          nullptr);
    bool ok = st != MPQE_OK || (u2[1] == 0 && u2[2] == 0);
    for (int s = 0; ok && st == MPQE_OK && s < 5; ++s) ok = u2[s] <= 2ull * lens_p[s] * lens_n[s];
    return verdict("auc_segments", st, ok);
}

int gqe_mixed_case(int form) {
    const int64_t D = 48, rows = 24, F = 3, B = 37;
    const float *tables[2] = {floats16(rows * D), floats16(rows * D)};
    const int64_t table_rows[2] = {rows, rows};
    const float *mats[4] = {floats16(D * D), floats16(D * D), floats16(D * D), floats16(D * D)};
    std::vector<int32_t> progs(F * MPQE_GQE_PROG_INTS, -1);
    for (int f = 0; f < F; ++f) {
        int32_t *p = progs.data() + f * MPQE_GQE_PROG_INTS;
        p[0] = form;
        p[1] = form ? 2 : 1;
        p[2] = 0;
        p[5] = 0;
        p[6] = f % 2;
        p[7] = 0;
        p[27] = 0;
        for (int b = 0; b < p[1]; ++b) {
            p[8 + 5 * b] = (f + b) % 2;
            p[9 + 5 * b] = form ? 1 : 2;
            for (int s = 0; s < p[9 + 5 * b]; ++s) p[10 + 5 * b + s] = 2 * ((f + b + s) % 4) + form;
        }
    }
    std::vector<int64_t> fo(B), neg_off(B + 1, 0), targets(B), anchors(2 * B);
    for (int64_t q = 0; q < B; ++q) {
        fo[q] = (q / 5) % F;
        neg_off[q + 1] = neg_off[q] + (q * 7) % 19;
        targets[q] = (q * 5) % rows;
        anchors[q] = (q * 3) % rows;
        anchors[B + q] = (q * 11) % rows;
    }
    const int64_t total = neg_off[B], n = B + total;
    std::vector<int64_t> tnodes(n), qrow(n);
    for (int64_t q = 0; q < B; ++q) {
        tnodes[q] = targets[q];
        qrow[q] = q;
        for (int64_t j = neg_off[q]; j < neg_off[q + 1]; ++j) {
            tnodes[B + j] = (j * 13) % rows;
            qrow[B + j] = q;
        }
    }
    std::vector<float> scores(n, NAN);
    int32_t err = 0;
    const size_t need = mpqe_gqe_mixed_desc_bytes(F);
    void *desc = exact(need);
    int st = mpqe_gqe_mixed_desc_build(progs.data(), F, tables, table_rows, 2, mats, 4, D, desc, need, nullptr);
    if (st != MPQE_OK) return verdict("gqe_mixed: descriptors", st, true);
    if (form == 0)
        st = mpqe_gqe_fwd_mixed(progs.data(), F, desc, need, nullptr, 0, D, fo.data(), B, tnodes.data(), n, anchors.data(), B,
                                qrow.data(), nullptr, n, 1e-8f, scores.data(), &err, nullptr);
    else
        st = mpqe_gqe_fwd_mixed(progs.data(), F, desc, need, nullptr, 0, D, fo.data(), B, anchors.data(), B, tnodes.data(), n,
                                nullptr, neg_off.data(), n, 1e-8f, scores.data(), &err, nullptr);
    bool ok = err == 0;
    for (float x : scores) ok = ok && std::isfinite(x) && std::fabs(x) <= 1.0001f;
    return verdict(form ? "gqe_mixed (intersection form)" : "gqe_mixed (chain form)", st, ok);
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s case off\n", argv[0]);
        return 2;
    }
    const std::string c = argv[1];
    g_off = atoi(argv[2]);
    if (c == "auc_segments") return auc_segments_case();
    if (c == "gqe_mixed") return gqe_mixed_case(0) | gqe_mixed_case(1);
    fprintf(stderr, "unknown case %s\n", c.c_str());
    return 2;
}
