// TEST INFRASTRUCTURE ONLY -- a stand-alone host program over the emulator build of the kernel sources (tests/emu): one
// level-form fused step (mpqe_step_forward_backward) with chosen operand groups one float (4 bytes) off a 16-byte boundary.
// Built with -fsanitize=alignment,address by tools/step_operand_sweep.sh, which runs it once per (dimension class, group):
// a 16-byte access the host chose for a pointer it never looked at is reported with its source line. The results are not
// compared with anything here (tests/test_step_operands.py does that); the program only asks for status 0, a clear error
// word and finite outputs.
//   step_operand_sweep D group [zero] [readout]
//     D        embedding dimension (64 / 128 / 256 run with MPQE_STEP_NO_CHAIN: the level form)
//     group    none | all | tables | mode_emb | basis_root | bias | readout | g_tables | g_mode_emb | g_basis | g_root |
//              g_bias | g_readout | outputs
//     zero     1: MPQE_STEP_ZERO_GRADS (default 0: the gradients are accumulated)
//     readout  0 sum (default), 2 mp, 4 mlp, 5 targetmlp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mpqe_amd.h"

namespace {
std::string g_group;
unsigned g_rng = 12345u;
float rnd() {       // (-0.5, 0.5)
    g_rng = g_rng * 1664525u + 1013904223u;
    return (float)(g_rng >> 8) / 16777216.f - 0.5f;
}
bool off(const char *group) { return g_group == "all" || g_group == group; }

// n floats, 16-byte aligned or (off) one float past a 16-byte boundary; the arena lives until exit
float *floats(size_t n, const char *group, float scale, float fill = NAN) {
    float *raw = static_cast<float *>(aligned_alloc(64, (n + 16 + 15) / 16 * 16 * sizeof(float)));
    float *p = raw + (off(group) ? 1 : 0);
    for (size_t i = 0; i < n; ++i) p[i] = std::isnan(fill) ? scale * rnd() : fill;
    return p;
}
void *bytes256(size_t n) {
    void *p = aligned_alloc(256, (n + 511) / 256 * 256);
    memset(p, 0, (n + 511) / 256 * 256);
    return p;
}
struct Template { int type, edges, vars, anchors; };       // (vars: the variable nodes, the target among them)
const Template kTemplates[] = {{MPQE_Q_3INTER_CHAIN, 3, 2, 2}, {MPQE_Q_2CHAIN, 2, 2, 1}, {MPQE_Q_1CHAIN, 1, 1, 1},
                               {MPQE_Q_3CHAIN_INTER, 3, 2, 2}, {MPQE_Q_3INTER, 3, 1, 3}};
}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s D group [zero] [readout]\n", argv[0]);
        return 2;
    }
    const int D = atoi(argv[1]);
    g_group = argv[2];
    const int zero = argc > 3 ? atoi(argv[3]) : 0, readout = argc > 4 ? atoi(argv[4]) : MPQE_READOUT_SUM;
    const bool learned = readout >= MPQE_READOUT_MLP;
    const int L = 2, R = 3, modes = 2, rows = 7, nb = 5;
    // whole K-steps (every batch a multiple of 32 rows) where the dimension allows LD_FAST, ragged sizes elsewhere
    const int sizes_fast[nb] = {32, 64, 32, 32, 32}, sizes_ragged[nb] = {5, 33, 1, 7, 32};
    const int *sizes = D % 64 == 0 ? sizes_fast : sizes_ragged;

    mpqe_step_params_t P;
    mpqe_step_grads_t G;
    memset(&P, 0, sizeof(P));
    memset(&G, 0, sizeof(G));
    P.dim = D; P.num_layers = L; P.num_relations = R; P.num_modes = modes; P.readout = readout;
    P.flags = MPQE_STEP_NO_CHAIN | (zero ? MPQE_STEP_ZERO_GRADS : 0);
    const float g0 = zero ? 7.5f : 0.f;
    std::vector<int64_t> node_map((size_t)modes * (rows - 1) + 1, -1);
    for (int m = 0; m < modes; ++m) {
        P.tables[m] = floats((size_t)rows * D, "tables", 1.f);
        P.table_rows[m] = rows;
        G.tables[m] = floats((size_t)rows * D, "g_tables", 0.f, g0);
        for (int r = 0; r < rows - 1; ++r) node_map[(size_t)m * (rows - 1) + r] = r;
    }
    P.node_map = node_map.data(); P.node_map_len = (int64_t)node_map.size();
    P.mode_emb = floats((size_t)modes * D, "mode_emb", 1.f);
    G.mode_emb = floats((size_t)modes * D, "g_mode_emb", 0.f, g0);
    const float bound = 3.f / std::sqrt((float)(R * D));
    for (int l = 0; l < L; ++l) {
        P.basis[l] = floats((size_t)R * D * D, "basis_root", 2 * bound);
        P.root[l] = floats((size_t)D * D, "basis_root", 2 * bound);
        P.bias[l] = floats(D, "bias", 2 * bound);
        G.basis[l] = floats((size_t)R * D * D, "g_basis", 0.f, g0);
        G.root[l] = floats((size_t)D * D, "g_root", 0.f, g0);
        G.bias[l] = floats(D, "g_bias", 0.f, g0);
    }
    if (learned) {
        const size_t kin = readout == MPQE_READOUT_TARGETMLP ? 2 * (size_t)D : (size_t)D;
        P.readout_w0 = floats(D * kin, "readout", 1.f / std::sqrt((float)kin)); P.readout_b0 = floats(D, "readout", 0.1f);
        P.readout_w2 = floats((size_t)D * D, "readout", 1.f / std::sqrt((float)D)); P.readout_b2 = floats(D, "readout", 0.1f);
        G.readout_w0 = floats(D * kin, "g_readout", 0.f, g0); G.readout_b0 = floats(D, "g_readout", 0.f, g0);
        G.readout_w2 = floats((size_t)D * D, "g_readout", 0.f, g0); G.readout_b2 = floats(D, "g_readout", 0.f, g0);
        P.readout_scatter = MPQE_SCATTER_ADD; P.readout_weight_decay = 1e-3f;
    }
    mpqe_step_batch_t B[nb];
    memset(B, 0, sizeof(B));
    std::vector<int64_t> anchors, targets, negs;
    long long graphs = 0;
    for (int i = 0; i < nb; ++i) {
        const Template &t = kTemplates[i];
        B[i].query_type = t.type; B[i].num_passes = L; B[i].batch_size = sizes[i]; B[i].target_mode = i % modes;
        B[i].weight = 1.f / (float)(i + 1);
        for (int e = 0; e < t.edges; ++e) B[i].edge_type[e] = (i + e) % R;
        for (int v = 0; v < t.vars; ++v) B[i].var_ids[v] = (i + v) % modes;
        for (int a = 0; a < t.anchors; ++a) B[i].anchor_mode[a] = (i + a) % modes;
        for (int a = 0; a < t.anchors; ++a)
            for (int g = 0; g < sizes[i]; ++g) anchors.push_back(((i + a) % modes) * (rows - 1) + (g + a) % (rows - 1));
        for (int g = 0; g < sizes[i]; ++g) {
            targets.push_back((i % modes) * (rows - 1) + g % (rows - 1));
            negs.push_back((i % modes) * (rows - 1) + (g + 3) % (rows - 1));
        }
        graphs += sizes[i];
    }
    float *loss = floats(1 + nb, "outputs", 0.f, -1.f);
    float *sp = floats((size_t)graphs, "outputs", 0.f, -1.f), *sn = floats((size_t)graphs, "outputs", 0.f, -1.f);
    const size_t wsb = mpqe_step_workspace_bytes(&P, B, nb, nullptr), dsb = mpqe_step_desc_bytes(&P, B, nb, nullptr);
    if (wsb == 0 || dsb == 0) {
        fprintf(stderr, "D %d %s: the size queries refuse the step\n", D, g_group.c_str());
        return 3;
    }
    void *ws = bytes256(wsb), *desc = bytes256(dsb);
    int32_t *err = static_cast<int32_t *>(bytes256(4));
    for (int backward = 1; backward >= 0; --backward) {        // a whole step, then a forward-only one
        const int st = mpqe_step_forward_backward(&P, B, nb, anchors.data(), targets.data(), negs.data(), 1.f, &G, backward, loss,
                                                  sp, sn, desc, dsb, backward, ws, wsb, err, nullptr, nullptr, 0, nullptr, nullptr);
        if (st != MPQE_OK || *err != 0 || !std::isfinite(loss[0])) {
            fprintf(stderr, "D %d %s backward %d: status %d, error word %d, loss %g\n", D, g_group.c_str(), backward, st, *err, loss[0]);
            return 4;
        }
    }
    double sum = 0;
    for (int l = 0; l < L; ++l)
        for (size_t i = 0; i < (size_t)D * D; ++i) sum += std::fabs(G.root[l][i]) + std::fabs(G.basis[l][i]);
    for (int i = 0; i < modes * D; ++i) sum += std::fabs(G.mode_emb[i]) + std::fabs(G.tables[0][i]);
    for (long long g = 0; g < graphs; ++g) sum += std::fabs(sp[g]) + std::fabs(sn[g]);
    if (!std::isfinite(sum)) {
        fprintf(stderr, "D %d %s: a gradient or score is not finite\n", D, g_group.c_str());
        return 5;
    }
    printf("D %d %s zero %d readout %d: ok (loss %.6f)\n", D, g_group.c_str(), zero, readout, loss[0]);
    return 0;
}
