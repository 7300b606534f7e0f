// TEST INFRASTRUCTURE ONLY -- a stand-alone host program over the emulator build of the kernel sources (tests/emu): entry
// points that take a workspace or a plan sized by an mpqe_*_bytes function, with that buffer EXACTLY the returned size --
// the inside of a heap block whose other bytes are poisoned -- and every byte 0xFF when the call starts. Built with
// -fsanitize=alignment,address by tools/workspace_sweep.sh:
// one byte read or written past the size the library asked for, or a 16-byte access to a buffer the host never looked at,
// is reported with its source line. Results are not compared with anything here (tests/test_workspace_bounds.py does
// that); the program asks for the expected status and finite outputs.
//   workspace_sweep case off
//     case  rank | rank_strips | general | general64 | linear | template | layernorm | scatter | rows
//     off   0: buffers 256-byte aligned; 4: every library-sized buffer 4 bytes past a 256-byte boundary -- the call may
//           then refuse (MPQE_ERR_INVALID_ARG / MPQE_ERR_WORKSPACE) or run, and must not make a misaligned wide access
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
std::vector<float> floats(size_t n, float scale = 1.f) {
    std::vector<float> v(n);
    for (auto &x : v) x = scale * rnd();
    return v;
}
// exactly n bytes, every byte 0xFF, `g_off` bytes past a 256-byte boundary; what lies in front of and behind them in their
// heap block is poisoned: the sanitizer reports the first byte touched outside
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
bool finite(const std::vector<float> &v) {
    for (float x : v)
        if (!std::isfinite(x)) return false;
    return true;
}
int verdict(const char *what, int st, bool ok) {
    const bool refused = g_off && (st == MPQE_ERR_INVALID_ARG || st == MPQE_ERR_WORKSPACE);
    if (refused) {
        printf("%s: refused (%d)\n", what, st);
        return 0;
    }
    if (st != MPQE_OK || !ok) {
        printf("%s: status %d, outputs %s\n", what, st, ok ? "finite" : "NOT finite");
        return 1;
    }
    printf("%s: ok\n", what);
    return 0;
}

int rank_case(int64_t Q, int64_t N, int64_t D, int k) {
    auto q = floats(Q * D), t = floats(N * D);
    std::vector<int64_t> target(Q), rows(Q * k), rank(Q);
    for (int64_t i = 0; i < Q; ++i) target[i] = (i * 7) % N;
    std::vector<float> sc(Q * k), ts(Q);
    int32_t err = 0;
    const size_t need = mpqe_rank_workspace_bytes(Q, N, D, k);
    void *ws = exact(need);
    const int st = mpqe_rank_entities(q.data(), Q, t.data(), N, D, 1e-8f, target.data(), nullptr, nullptr, 0, k, rows.data(),
                                      sc.data(), rank.data(), ts.data(), ws, need, &err, nullptr);
    return verdict("rank", st, err == 0 && finite(ts));
}

int general_case(int64_t Din, int64_t Dout) {
    const int64_t Nn = 130, E = 400, R = 3;
    std::vector<int64_t> ei(2 * E), et(E);
    for (int64_t e = 0; e < E; ++e) {
        ei[e] = (e * 37) % Nn;
        ei[E + e] = e < 110 ? 3 : (e * 11) % Nn;
        et[e] = e % 7 == 0 ? 2 : 0;         // relation 1: no edge
    }
    int32_t err = 0;
    const size_t pb = mpqe_rgcn_plan_bytes(Nn, E, R), pw = mpqe_rgcn_plan_workspace_bytes(Nn, E, R);
    void *plan = exact(pb), *pws = exact(pw);
    int st = mpqe_rgcn_plan_build(ei.data(), et.data(), Nn, E, R, plan, pb, pws, pw, &err, nullptr);
    if (st != MPQE_OK) return verdict("general: plan", st, true);
    auto x = floats(Nn * Din), basis = floats(R * Din * Dout, 0.3f), root = floats(Din * Dout, 0.3f), bias = floats(Dout);
    auto g = floats(Nn * Dout);
    std::vector<float> out(Nn * Dout), gx(Nn * Din), gb(R * Din * Dout), gr(Din * Dout), gbi(Dout);
    const size_t wf = mpqe_rgcn_general_workspace_bytes(Nn, E, R, Din, Dout, 0);
    void *ws = exact(wf);
    st = mpqe_rgcn_general_fwd(plan, Nn, E, R, x.data(), basis.data(), root.data(), bias.data(), Din, Dout, 1, out.data(),
                               nullptr, ws, wf, nullptr);
    if (st != MPQE_OK || !finite(out)) return verdict("general: forward", st, finite(out));
    const size_t wb = mpqe_rgcn_general_workspace_bytes(Nn, E, R, Din, Dout, 1);
    void *ws2 = exact(wb);
    st = mpqe_rgcn_general_bwd(plan, Nn, E, R, x.data(), out.data(), nullptr, g.data(), basis.data(), root.data(), Din, Dout,
                               1, 1, gx.data(), gb.data(), gr.data(), gbi.data(), ws2, wb, nullptr);
    return verdict("general", st, err == 0 && finite(gx) && finite(gb) && finite(gr) && finite(gbi));
}

int linear_case() {
    const int64_t rows = 70, din = 48, dout = 20;
    auto x = floats(rows * din), W = floats(dout * din, 0.2f), y = floats(rows * dout), g = floats(rows * dout);
    std::vector<float> gx(rows * din), gW(dout * din), gb(dout);
    const size_t need = mpqe_linear_bwd_workspace_bytes(rows, din, dout);
    void *ws = exact(need);
    const int st = mpqe_linear_bwd(x.data(), rows, W.data(), din, y.data(), g.data(), din, dout, 1, 1, gx.data(), gW.data(),
                                   din, gb.data(), ws, need, nullptr);
    return verdict("linear_bwd", st, finite(gx) && finite(gW) && finite(gb));
}

int template_case() {
    const int64_t B = 67, Din = 40, Dout = 24, R = 5, N = 4;
    const int64_t et[3] = {1, 4, 1};
    auto x = floats(B * N * Din), out = floats(B * N * Dout), g = floats(B * N * Dout);
    auto basis = floats(R * Din * Dout, 0.3f), root = floats(Din * Dout, 0.3f);
    std::vector<float> gx(B * N * Din), gb(R * Din * Dout, 0.f), gr(Din * Dout, 0.f), gbi(Dout, 0.f);
    const size_t need = mpqe_rgcn_template_bwd_workspace_bytes(MPQE_Q_3INTER_CHAIN, B, Din, Dout);
    void *ws = exact(need);
    const int st = mpqe_rgcn_template_bwd(MPQE_Q_3INTER_CHAIN, B, et, x.data(), out.data(), g.data(), basis.data(), R,
                                          root.data(), Din, Dout, 1, gx.data(), gb.data(), gr.data(), gbi.data(), ws, need,
                                          nullptr);
    return verdict("template_bwd", st, finite(gx) && finite(gb) && finite(gr) && finite(gbi));
}

int layernorm_case() {
    const int64_t rows = 9, D = 260;
    auto x = floats(rows * D, 4.f), gamma = floats(D), beta = floats(D), gy = floats(rows * D);
    std::vector<float> y(rows * D), stats(rows * 2), gx(rows * D), gg(D, 0.f), gb(D, 0.f);
    int st = mpqe_layernorm_relu_fwd(x.data(), rows, D, gamma.data(), beta.data(), 1e-6f, 1, y.data(), stats.data(), nullptr);
    if (st != MPQE_OK) return verdict("layernorm: forward", st, true);
    const size_t need = mpqe_layernorm_relu_bwd_workspace_bytes(rows, D);
    void *ws = exact(need);
    st = mpqe_layernorm_relu_bwd(gy.data(), x.data(), y.data(), rows, D, gamma.data(), stats.data(), 1e-6f, 1, gx.data(),
                                 gg.data(), gb.data(), ws, need, nullptr);
    return verdict("layernorm_bwd", st, finite(gx) && finite(gg) && finite(gb));
}

int scatter_case() {
    const int64_t n = 150, D = 5, size = 65;
    auto src = floats(n * D), g = floats(size * D);
    std::vector<int64_t> index(n), arg(size * D);
    for (int64_t i = 0; i < n; ++i) index[i] = (i * 13) % size % 3 == 1 ? 0 : (i * 13) % size;
    std::vector<float> out(size * D), gs(n * D);
    int32_t err = 0;
    const size_t need = mpqe_scatter_workspace_bytes(n, size);
    void *ws = exact(need);
    int st = mpqe_scatter_fwd(MPQE_SCATTER_MEAN, src.data(), index.data(), n, D, size, out.data(), arg.data(), ws, need, &err,
                              nullptr);
    if (st != MPQE_OK || !finite(out)) return verdict("scatter: forward", st, finite(out));
    st = mpqe_scatter_bwd(MPQE_SCATTER_MEAN, g.data(), index.data(), arg.data(), n, D, size, gs.data(), ws, need, nullptr);
    return verdict("scatter mean", st, err == 0 && finite(gs));
}

int rows_case() {
    const int64_t n = 257;
    const int row_bits = 12, key_bits = 17;
    std::vector<uint64_t> keys(n);
    for (int64_t i = 0; i < n; ++i) keys[i] = i == 100 ? ~0ull : (uint64_t)(((i * 5) % 64) | ((i % 2) << row_bits));
    const size_t pb = mpqe_rows_plan_bytes(n), wb = mpqe_rows_plan_workspace_bytes(n, key_bits);
    void *plan = exact(pb), *ws = exact(wb);
    int st = mpqe_rows_plan_build(keys.data(), n, row_bits, key_bits, plan, pb, ws, wb, nullptr);
    if (st != MPQE_OK) return verdict("rows plan", st, true);
    const int64_t D = 16;
    auto rows = floats(n * D);
    std::vector<float> t0(300 * D, 0.f), t1(200 * D, 0.f);
    float *tabs[2] = {t0.data(), t1.data()};
    st = mpqe_table_rows_sum(plan, n, rows.data(), D, tabs, 2, 0, nullptr);
    return verdict("rows plan + sum", st, finite(t0) && finite(t1));
}
}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s case off\n", argv[0]);
        return 2;
    }
    const std::string c = argv[1];
    g_off = atoi(argv[2]);
    if (c == "rank") return rank_case(65, 257, 48, 128);
    if (c == "rank_strips") return rank_case(3, 8300, 8, 65);
    if (c == "general") return general_case(10, 6);
    if (c == "general64") return general_case(128, 64);
    if (c == "linear") return linear_case();
    if (c == "template") return template_case();
    if (c == "layernorm") return layernorm_case();
    if (c == "scatter") return scatter_case();
    if (c == "rows") return rows_case();
    fprintf(stderr, "unknown case %s\n", c.c_str());
    return 2;
}
