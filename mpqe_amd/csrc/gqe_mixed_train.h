// Training on queries of different formulas at once: the states of mpqe_gqe_fwd_mixed_save and mpqe_gqe_bwd_mixed.
// Included by gqe.hip after the mixed forward (GqeDev, GqeMixDesc, the gq_* helpers and gq_mix_formula are its).
//
// The workspace (mpqe_gqe_mixed_train_workspace_bytes; floats, every block a multiple of 256 bytes), all indexed by P row
// of the concatenation (Rp16 = P rows rounded up to 16), slot k = the k-th site the query type uses, in site order:
//   X[k], dY[k]  [Rp16, D] each  the input rows of the site and the gradient of its output; a vector site keeps its
//                                 gradient TERM in dY[k] (translate: dy, scale: x * dy) and X[k] only under scale
//   T[b], Pfin   [Rp16, D]       as mpqe_gqe_fwd
//   GE           [nb * Rp16 + n, D], key / etab [nb * Rp + n] int64 / pointer: the looked-up rows' gradients, their
//                                 (table index << 40 | row) keys and their tables
//   ptrs         [num_tables + num_mats] the caller's gradient buffers (one copy per call from a host image)
//   ckey / cval, skey / sval [slots * Rp]  the contributions (site slot, P row), unsorted and sorted by parameter index;
//                                 value = (contribution number << 1) | transposition
//   seg          [num_mats + 1][2] every parameter's segment of the sorted list
//   the radix sort's scratch
// A stretch writes only its own rows [first, end) of every state; a row no stretch of a valid formula owns is never read:
// its contributions carry the key num_mats (they sort behind every parameter) and its entries the key -1.
//
// State gradients (gqe_bwd_mixed_kernel): gqe_bwd_kernel's body on a stretch. A row's arithmetic depends neither on its
// tile row nor on its tile's other rows (gq_mm's sum over k is per output element, everything else is per row), so every
// dY and GE row is bit for bit what mpqe_gqe_bwd computes when the query's run is handed to it alone. The kernel also
// writes the keys of the looked-up rows it owns (mpqe_gqe_bwd's gqe_keys_kernel).
//
// Parameter gradients (gqe_mix_param_kernel; mix_grad_core.h's param_reduce / vec_reduce with chunks of
// MPQE_GQE_MIX_GRAD_CHUNK): the key is the parameter index; the list starts site-major, row-minor, so a parameter's
// segment is ordered by site, then row. A matrix contribution's A / B rows are its X / dY rows, swapped for a transposed
// site; a vector contribution's row is its dY row (the term). Every order is a function of (formula_of, programmes) alone.
//
// Table rows (gqe_rows_mixed_kernel; rows_reduce): the entries are the branch sources in branch order, then the E row of
// every pair, as in mpqe_gqe_bwd, with the table of every entry and the gradient buffer of every table index.
#pragma once
#include "radix_sort.h"

struct GqeMixIdx {
    int tab[4];             // table index of the branch sources and of the E side (-1: slot unused)
    int par[GQ_SITES];      // parameter index of every site (-1: site unused)
};

struct GqeMixTrain {
    const GqeMixDesc *desc;
    const GqeMixIdx *idx;
    const long long *fo;
    long long B;
    int F, num_tables, num_mats, nus;
    unsigned vecmask;                  // bit k: slot k holds a vector
    unsigned long long us;             // 4 bits per slot: its site
    long long blk;                     // Rp16 * D: slot k keeps X at 2 k blk, dY at (2 k + 1) blk
    long long etab_off, ptr_off, ckey_off, cval_off, skey_off, sval_off, seg_off;
    long long NC;
};

struct GqeMixLayout {
    GqeMixTrain Tn;
    long long n_ent;
    size_t sort_off, total;
};

// the key of a looked-up row: (table index << 40) | row; -1 where the table wants no gradient or the id is bad
__device__ __forceinline__ long long gq_mix_key(const GqeDev &G, const GqeMixTrain &Tn, int tidx, int slot, long long id) {
    float *const *gt = reinterpret_cast<float *const *>(G.ws + Tn.ptr_off);
    if (tidx < 0 || tidx >= Tn.num_tables || !gt[tidx]) return -1;
    const long long row = lookup_row(G.node_map, G.map_len, id, G.tab_rows[slot], nullptr);      // (flagged by the forward)
    return row < 0 ? -1 : (((long long)tidx << 40) | row);
}

// the E entry of pair r: its key and table
__device__ __forceinline__ void gq_mix_e_entry(const GqeDev &G, const GqeMixTrain &Tn, int tidx, long long r) {
    long long e = r, key = -1;
    if (G.form == 0) {
        e = G.qrow[r];
        if (e < 0 || e >= G.Re) e = -1;
    }
    if (e >= 0) key = gq_mix_key(G, Tn, tidx, 3, G.e_ids[e]);
    const long long at = (long long)G.nb * G.Rp + r;
    reinterpret_cast<long long *>(G.ws + G.key_off)[at] = key;
    reinterpret_cast<const float **>(G.ws + Tn.etab_off)[at] = G.tab[3];
}

// the backward of one vector site on a stretch's tile of dY, in place: the rows' terms of the vector's gradient (translate:
// dy, scale: x * dy) -> rows [first, first + cnt) of `term`; scale: dX = dY * v
__device__ __forceinline__ void gq_vec_bwd_rows(float *tile, int LDX, const float *v, const float *X, float *term,
                                                long long first, int cnt, int D, int op) {
    const int per = D / 4;
    for (int e = threadIdx.x; e < GQ_ROWS * per; e += 256) {
        const int i = e / per, c = (e % per) * 4;
        f32x4 g = *reinterpret_cast<const f32x4 *>(tile + i * LDX + c);
        if (i < cnt) {
            f32x4 t = g;
            if (op == 2) {
                const f32x4 x = gload4(X + (first + i) * D + c);
#pragma unroll
                for (int u = 0; u < 4; ++u) t[u] = x[u] * g[u];
            }
            *reinterpret_cast<f32x4 *>(term + (first + i) * D + c) = t;
        }
        if (op == 2) {
            const f32x4 w = gload4(v + c);
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] *= w[u];
            *reinterpret_cast<f32x4 *>(tile + i * LDX + c) = g;
        }
    }
}

template <int DOT>
__global__ __launch_bounds__(256) void gqe_bwd_mixed_kernel(GqeDev G, GqeMixTrain Tn, const float *__restrict__ gs) {
    __shared__ __attribute__((aligned(16))) float lds[3 * GQ_ROWS * GQ_LDXMAX];
    const int D = G.D, LDX = D + 4, per = D / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long first, end;
    int fi;
    if (!gq_mix_stretch(G, Tn.fo, Tn.B, Tn.F, first, end, fi)) return;
    fi = __builtin_amdgcn_readfirstlane(fi);
    if (fi < 0) {
        // (no state, no contribution, no entry: the contributions' keys and the entries' keys say so)
        if (threadIdx.x == 0) flag_error(G.err, MPQE_FLAG_BAD_INDEX);
        return;
    }
    const GqeMixDesc &M = Tn.desc[fi];
    const GqeMixIdx &I = Tn.idx[fi];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        G.tab[t] = M.tab[t];
        G.tab_rows[t] = M.tab_rows[t];
    }
    const int cnt = (int)(end - first);
    float *cur = lds, *nxt = lds + GQ_ROWS * LDX, *ga = lds + 2 * GQ_ROWS * LDX;
    float *GE = G.ws + G.ge_off;
    const long long ge_e0 = (long long)G.nb * G.Rp16;      // first E entry row of GE

    // scores: the gradient of the scored rows -> cur (rows past the stretch: zeros), of the E rows -> GE
    for (int i = wave; i < GQ_ROWS; i += 4) {
        const long long q = first + i;
        f32x4 gp = {0.f, 0.f, 0.f, 0.f};
        if (q < end) {
            f32x4 p = {0.f, 0.f, 0.f, 0.f};
            if (lane * 4 < D) p = gload4(G.ws + G.pfin_off + q * D + lane * 4);
            if (G.form == 0) {
                f32x4 ge;
                const float g = gs[q];
                gq_score<DOT>(G, p, gq_e_row(G, q, lane), &g, &gp, &ge);
                if (lane * 4 < D) *reinterpret_cast<f32x4 *>(GE + (ge_e0 + q) * D + lane * 4) = ge;
                if (lane == 0) gq_mix_e_entry(G, Tn, I.tab[3], q);
            } else {
                long long lo, hi;
                gq_neg_range(G, q, lane, lo, hi);
                for (long long r = q;;) {
                    f32x4 g1, ge;
                    const float g = gs[r];
                    gq_score<DOT>(G, p, gq_e_row(G, r, lane), &g, &g1, &ge);
#pragma unroll
                    for (int u = 0; u < 4; ++u) gp[u] += g1[u];
                    if (lane * 4 < D) *reinterpret_cast<f32x4 *>(GE + (ge_e0 + r) * D + lane * 4) = ge;
                    if (lane == 0) gq_mix_e_entry(G, Tn, I.tab[3], r);
                    r = r == q ? lo : r + 1;
                    if (r >= hi) break;
                }
            }
        }
        if (lane * 4 < D) *reinterpret_cast<f32x4 *>(cur + i * LDX + lane * 4) = gp;
    }
    __syncthreads();

    for (int s = G.ntail - 1; s >= 0; --s) {
        const int site = GQ_SITE_TAIL + s;
        if (G.op) {
            gq_vec_bwd_rows(cur, LDX, M.w[site], G.ws + gq_mix_x_off(G, site), G.ws + gq_mix_dy_off(G, site), first, cnt, D, G.op);
            __syncthreads();
            continue;
        }
        gq_store_rows(cur, LDX, G.ws + gq_mix_dy_off(G, site), first, cnt, D);
        gq_mm(cur, nxt, M.w[site], D, LDX, !M.T[site], 0);
        __syncthreads();
        float *t = cur; cur = nxt; nxt = t;
    }
    if (G.nb >= 2) {
        if (G.has_post) {
            gq_store_rows(cur, LDX, G.ws + gq_mix_dy_off(G, GQ_SITE_POST), first, cnt, D);
            gq_mm(cur, nxt, M.w[GQ_SITE_POST], D, LDX, 0, 0);
            __syncthreads();
            float *t = cur; cur = nxt; nxt = t;
        }
        float *t = cur; cur = ga; ga = t;       // ga: the gradient of the aggregate, kept over the branches
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        if (b >= G.nb) break;
        if (G.nb >= 2) {
            for (int e = threadIdx.x; e < GQ_ROWS * per; e += 256) {
                const int i = e / per, c = (e % per) * 4;
                const f32x4 g = *reinterpret_cast<const f32x4 *>(ga + i * LDX + c);
                f32x4 tv[3];
                for (int k = 0; k < G.nb; ++k) {
                    tv[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (i < cnt) tv[k] = gload4(G.ws + gq_mix_t_off(G, k) + (first + i) * D + c);
                }
                f32x4 v;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float x;
                    if (G.agg) {
                        // min: the gradient goes to the first branch that holds the minimum
                        int win = 0;
                        float m = tv[0][u];
                        for (int k = 1; k < G.nb; ++k)
                            if (tv[k][u] < m) {
                                m = tv[k][u];
                                win = k;
                            }
                        x = win == b ? g[u] : 0.f;
                    } else {
                        x = g[u] / (float)G.nb;
                    }
                    if (G.has_pre && !(tv[b][u] > 0.f)) x = 0.f;
                    v[u] = x;
                }
                *reinterpret_cast<f32x4 *>(cur + i * LDX + c) = v;
            }
            __syncthreads();
            if (G.has_pre) {
                gq_store_rows(cur, LDX, G.ws + gq_mix_dy_off(G, GQ_SITE_PRE + b), first, cnt, D);
                gq_mm(cur, nxt, M.w[GQ_SITE_PRE + b], D, LDX, 0, 0);
                __syncthreads();
                float *t = cur; cur = nxt; nxt = t;
            }
        }
        for (int s = G.bn[b] - 1; s >= 0; --s) {
            const int site = 3 * b + s;
            if (G.op) {
                gq_vec_bwd_rows(cur, LDX, M.w[site], G.ws + gq_mix_x_off(G, site), G.ws + gq_mix_dy_off(G, site), first, cnt, D, G.op);
                __syncthreads();
                continue;
            }
            gq_store_rows(cur, LDX, G.ws + gq_mix_dy_off(G, site), first, cnt, D);
            gq_mm(cur, nxt, M.w[site], D, LDX, !M.T[site], 0);
            __syncthreads();
            float *t = cur; cur = nxt; nxt = t;
        }
        gq_store_rows(cur, LDX, GE + (long long)b * G.Rp16 * D, first, cnt, D);
        // the branch sources' entries
        if ((int)threadIdx.x < cnt) {
            const long long at = (long long)b * G.Rp + first + threadIdx.x;
            reinterpret_cast<long long *>(G.ws + G.key_off)[at] = gq_mix_key(G, Tn, I.tab[b], b, G.p_ids[at]);
            reinterpret_cast<const float **>(G.ws + Tn.etab_off)[at] = G.tab[b];
        }
        __syncthreads();
    }
}

// mpqe_gqe_bwd's entries with the table of every entry and the gradient buffer of every table index
struct GqeMixEntries : GqeEntries {
    const GqeMixTrain &Tn;
    __device__ __forceinline__ void tables(long long e, long long key, const float *&tab, float *&gtab) const {
        tab = reinterpret_cast<const float *const *>(G.ws + Tn.etab_off)[e];
        gtab = reinterpret_cast<float *const *>(G.ws + Tn.ptr_off)[key >> 40];
    }
};

__global__ __launch_bounds__(256) void gqe_rows_mixed_kernel(GqeDev G, GqeMixTrain Tn, long long n_ent) {
    rows_reduce(GqeMixEntries{{G}, Tn}, n_ent, G.D);
}

// contribution c = (slot k, P row): its parameter (num_mats: none) and (c << 1) | transposition
__global__ __launch_bounds__(256) void gqe_mix_ckeys_kernel(GqeDev G, GqeMixTrain Tn) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= Tn.NC) return;
    const unsigned k = (unsigned)(c / G.Rp);
    const long long row = c % G.Rp;
    const int site = (int)((Tn.us >> (4 * k)) & 15ull);
    const long long f = gq_mix_formula(G, Tn.fo, Tn.B, Tn.F, row);
    int key = Tn.num_mats, T = 0;
    if (f >= 0) {
        const int par = Tn.idx[f].par[site];
        if (par >= 0 && par < Tn.num_mats) key = par;
        T = Tn.desc[f].T[site] != 0;
    }
    reinterpret_cast<unsigned *>(G.ws + Tn.ckey_off)[c] = (unsigned)key;
    reinterpret_cast<int *>(G.ws + Tn.cval_off)[c] = (int)((c << 1) | T);
}

__global__ __launch_bounds__(256) void gqe_mix_seg_kernel(GqeDev G, GqeMixTrain Tn) {
    mix_seg(reinterpret_cast<const unsigned *>(G.ws + Tn.skey_off), reinterpret_cast<int *>(G.ws + Tn.seg_off), Tn.NC,
            (unsigned)Tn.num_mats);
}

// sorted value = (contribution number (slot k, P row) << 1) | transposition -> its rows of X[k] and dY[k]
struct GqeMixContrib {
    const float *S;
    unsigned Rp;
    long long blk;
    int D;
    __device__ __forceinline__ void rows(unsigned val, const float *&A, const float *&B) const {
        const unsigned ci = val >> 1, k = ci / Rp, row = ci % Rp;
        const float *X = S + 2ll * k * blk + (long long)row * D, *dY = X + blk;
        A = (val & 1u) ? dY : X;
        B = (val & 1u) ? X : dY;
    }
    __device__ __forceinline__ const float *term(unsigned val) const {
        const unsigned ci = val >> 1, k = ci / Rp, row = ci % Rp;
        return S + (2ll * k + 1) * blk + (long long)row * D;
    }
};

// workgroup = (parameter, strip of 16 gradient rows); a vector: the workgroup of strip 0
__global__ __launch_bounds__(256) void gqe_mix_param_kernel(GqeDev G, GqeMixTrain Tn) {
    const int D = G.D, nstrip = D / 16;
    const int par = blockIdx.x / nstrip, rs = blockIdx.x % nstrip;
    float *g = reinterpret_cast<float *const *>(G.ws + Tn.ptr_off)[Tn.num_tables + par];
    if (!g) return;
    const int *seg = reinterpret_cast<const int *>(G.ws + Tn.seg_off);
    const int lo = seg[2 * par], hi = seg[2 * par + 1];
    if (lo >= hi) return;
    const int *sval = reinterpret_cast<const int *>(G.ws + Tn.sval_off);
    const GqeMixContrib C = {G.ws, (unsigned)G.Rp, Tn.blk, D};
    if ((Tn.vecmask >> (((unsigned)sval[lo] >> 1) / C.Rp)) & 1u) {
        if (rs == 0) vec_reduce<MPQE_GQE_MIX_GRAD_CHUNK>(lo, hi, g, D, sval, C);
        return;
    }
    param_reduce<MPQE_GQE_MIX_GRAD_CHUNK>(lo, hi, rs, g, D, sval, C);
}

// ------------------------------------------------------------------------------------------------ host side
static inline size_t gqe_mixed_index_size(int64_t F) { return align_up((size_t)F * sizeof(GqeMixIdx), 256); }

extern "C" size_t mpqe_gqe_mixed_index_bytes(int64_t num_formulas) {
    if (num_formulas < 1 || num_formulas >= ((int64_t)1 << 24)) return 0;
    return gqe_mixed_index_size(num_formulas);
}

extern "C" int mpqe_gqe_mixed_index_build(const int32_t *progs_host, int64_t num_formulas, int num_tables, int num_mats,
                                          int64_t dim, void *index, size_t index_bytes, void *stream) {
    if (!progs_host || num_tables < 1 || num_mats < 0 || !index) return MPQE_ERR_INVALID_ARG;
    if (num_formulas < 1 || num_formulas >= ((int64_t)1 << 24)) return MPQE_ERR_INVALID_ARG;
    if ((uintptr_t)index % 256 != 0) return MPQE_ERR_INVALID_ARG;
    return mix_upload<GqeMixIdx>(index, (size_t)num_formulas, as_stream(stream), [&](GqeMixIdx *image) -> int {
        for (int64_t f = 0; f < num_formulas; ++f) {
            const int32_t *prog = progs_host + f * MPQE_GQE_PROG_INTS;
            GqeHost H;
            const int st = gqe_plan(prog, num_tables, num_mats, dim, 1, 1, 1, &H);
            if (st != MPQE_OK) return st;
            if (!gqe_mixed_same_shape(progs_host, prog)) return MPQE_ERR_INVALID_ARG;
            for (int t = 0; t < 4; ++t) image[f].tab[t] = t < 3 && t >= H.G.nb ? -1 : H.G.tmode[t];
            for (int s = 0; s < GQ_SITES; ++s) image[f].par[s] = H.site_mat[s];
        }
        return index_bytes < gqe_mixed_index_size(num_formulas) ? MPQE_ERR_WORKSPACE : MPQE_OK;
    });
}

// the shared programme + sizes -> device record and the training workspace's layout
static int gqe_mixed_train_plan(const int32_t *prog, int64_t num_formulas, int num_tables, int num_mats, int64_t dim,
                                int64_t p_rows, int64_t e_rows, int64_t n, GqeHost *H, GqeMixLayout *L) {
    if (num_tables < 1 || num_mats < 0 || num_tables > (1 << 20) || num_mats >= (1 << 30)) return MPQE_ERR_INVALID_ARG;
    if (num_formulas < 1 || num_formulas >= ((int64_t)1 << 24)) return MPQE_ERR_INVALID_ARG;
    const int st = gqe_plan(prog, num_tables, num_mats, dim, p_rows, e_rows, n, H);
    if (st != MPQE_OK) return st;
    GqeDev &G = H->G;
    memset(L, 0, sizeof(*L));
    GqeMixTrain &Tn = L->Tn;
    Tn.num_tables = num_tables;
    Tn.num_mats = num_mats;
    Tn.blk = G.Rp16 * dim;
    for (int s = 0; s < GQ_SITES; ++s) {
        G.x_off[s] = G.dy_off[s] = G.part_off[s] = -1;
        if (H->site_mat[s] < 0) continue;
        const int k = Tn.nus++;
        Tn.us |= (unsigned long long)s << (4 * k);
        const bool vec = gqe_vec_site(G.op, s);
        if (vec) Tn.vecmask |= 1u << k;
        if (!vec || G.op == 2) G.x_off[s] = 2ll * k * Tn.blk;
        G.dy_off[s] = (2ll * k + 1) * Tn.blk;
        G.save |= 1 << s;                  // (the kernels' gq_mix_x_off / gq_mix_dy_off / gq_mix_t_off read the mask)
    }
    Tn.NC = (long long)Tn.nus * p_rows;
    if (Tn.NC >= (1ll << 30)) return MPQE_ERR_UNSUPPORTED;
    long long off = 2ll * Tn.nus * Tn.blk;
    for (int b = 0; b < 3; ++b) {
        G.t_off[b] = -1;
        if (G.nb >= 2 && b < G.nb) {
            G.t_off[b] = off;
            off += Tn.blk;
        }
    }
    G.pfin_off = off;
    off += Tn.blk;
    G.ge_off = off;
    off += (long long)align_up((size_t)((long long)G.nb * G.Rp16 + n) * (size_t)dim, 64);
    L->n_ent = (long long)G.nb * p_rows + n;
    G.key_off = off;
    off += (long long)align_up((size_t)L->n_ent * 2, 64);
    Tn.etab_off = off;
    off += (long long)align_up((size_t)L->n_ent * 2, 64);
    Tn.ptr_off = off;
    off += (long long)align_up((size_t)(num_tables + num_mats) * 2, 64);
    const long long nc64 = (long long)align_up((size_t)Tn.NC, 64);
    Tn.ckey_off = off;
    Tn.cval_off = off + nc64;
    Tn.skey_off = off + 2 * nc64;
    Tn.sval_off = off + 3 * nc64;
    off += 4 * nc64;
    Tn.seg_off = off;
    off += (long long)align_up((size_t)(num_mats + 1) * 2, 64);
    L->sort_off = (size_t)off * 4;
    L->total = L->sort_off + radix_sort_tmp_bytes<unsigned>(Tn.NC);
    return MPQE_OK;
}

extern "C" size_t mpqe_gqe_mixed_train_workspace_bytes(const int32_t *prog_host, int64_t num_formulas, int num_tables,
                                                       int num_mats, int64_t p_rows, int64_t n, int64_t dim) {
    GqeHost H;
    GqeMixLayout L;
    if (!prog_host) return 0;
    const int64_t e_rows = prog_host[0] == 0 ? 1 : n;
    if (gqe_mixed_train_plan(prog_host, num_formulas, num_tables, num_mats, dim, p_rows, e_rows, n, &H, &L) != MPQE_OK) return 0;
    return L.total;
}

// the checks and the device record both mixed forwards and the mixed backward share; L == NULL: no workspace
static int gqe_mixed_call(const int32_t *prog_host, int64_t num_formulas, const void *desc, size_t desc_bytes, int num_tables,
                          int num_mats, const int64_t *node_map, int64_t node_map_len, int64_t dim, const int64_t *formula_of,
                          int64_t num_queries, const int64_t *p_ids, int64_t p_rows, const int64_t *e_ids, int64_t e_rows,
                          const int64_t *qrow, const int64_t *neg_off, int64_t n, float eps, void *workspace,
                          size_t workspace_bytes, int32_t *err, GqeHost *H, GqeMixLayout *L, bool *empty) {
    *empty = false;
    if (!prog_host || num_queries < 0 || node_map_len < 0) return MPQE_ERR_INVALID_ARG;
    if (num_formulas < 1 || num_formulas >= ((int64_t)1 << 24)) return MPQE_ERR_INVALID_ARG;
    if (!desc || (uintptr_t)desc % 256 != 0) return MPQE_ERR_INVALID_ARG;
    if (desc_bytes < gqe_mixed_desc_size(num_formulas)) return MPQE_ERR_WORKSPACE;
    if (num_queries == 0) {
        *empty = true;
        return n == 0 && p_rows == 0 && e_rows == 0 ? MPQE_OK : MPQE_ERR_INVALID_ARG;
    }
    if (L && (!workspace || (uintptr_t)workspace % 256 != 0)) return MPQE_ERR_INVALID_ARG;
    if (!formula_of || !p_ids || !e_ids) return MPQE_ERR_INVALID_ARG;
    const int st = L ? gqe_mixed_train_plan(prog_host, num_formulas, num_tables, num_mats, dim, p_rows, e_rows, n, H, L)
                     : gqe_plan(prog_host, -1, -1, dim, p_rows, e_rows, n, H);
    if (st != MPQE_OK) return st;
    GqeDev &G = H->G;
    // chain form: one anchor per query; intersection form: one P row per query
    if (G.form == 0 ? e_rows != num_queries : p_rows != num_queries) return MPQE_ERR_INVALID_ARG;
    if (G.form == 0 && !qrow) return MPQE_ERR_INVALID_ARG;
    if (G.form == 1 && G.n > G.Rp && !neg_off) return MPQE_ERR_INVALID_ARG;
    if (G.Rp16 / GQ_ROWS >= (1ll << 27)) return MPQE_ERR_UNSUPPORTED;
    if (L && workspace_bytes < L->total) return MPQE_ERR_WORKSPACE;
    G.node_map = (const long long *)node_map;
    G.map_len = node_map_len;
    G.p_ids = (const long long *)p_ids;
    G.e_ids = (const long long *)e_ids;
    G.qrow = (const long long *)qrow;
    G.neg_off = (const long long *)neg_off;
    G.eps = eps;
    G.err = err;
    G.ws = reinterpret_cast<float *>(workspace);
    if (L) {
        L->Tn.desc = reinterpret_cast<const GqeMixDesc *>(desc);
        L->Tn.fo = reinterpret_cast<const long long *>(formula_of);
        L->Tn.B = num_queries;
        L->Tn.F = (int)num_formulas;
    }
    return MPQE_OK;
}

template <int SAVE>
static int gqe_fwd_mixed_launch(const GqeDev &G, const void *desc, const int64_t *formula_of, int64_t num_queries,
                                int64_t num_formulas, float *scores, void *stream) {
    const dim3 grid((unsigned)(G.Rp16 / GQ_ROWS * 16));
    const GqeMixDesc *M = reinterpret_cast<const GqeMixDesc *>(desc);
    const long long *fo = reinterpret_cast<const long long *>(formula_of);
    if (G.dot)
        hipLaunchKernelGGL((gqe_fwd_mixed_kernel<1, SAVE>), grid, dim3(256), 0, as_stream(stream), G, M, fo,
                           (long long)num_queries, (int)num_formulas, scores);
    else
        hipLaunchKernelGGL((gqe_fwd_mixed_kernel<0, SAVE>), grid, dim3(256), 0, as_stream(stream), G, M, fo,
                           (long long)num_queries, (int)num_formulas, scores);
    return mpqe_launch_status();
}

extern "C" int mpqe_gqe_fwd_mixed(const int32_t *prog_host, int64_t num_formulas, const void *desc, size_t desc_bytes,
                                  const int64_t *node_map, int64_t node_map_len, int64_t dim, const int64_t *formula_of,
                                  int64_t num_queries, const int64_t *p_ids, int64_t p_rows, const int64_t *e_ids,
                                  int64_t e_rows, const int64_t *qrow, const int64_t *neg_off, int64_t n, float eps,
                                  float *scores, int32_t *err, void *stream) {
    GqeHost H;
    bool empty;
    const int st = gqe_mixed_call(prog_host, num_formulas, desc, desc_bytes, 0, 0, node_map, node_map_len, dim, formula_of,
                                  num_queries, p_ids, p_rows, e_ids, e_rows, qrow, neg_off, n, eps, nullptr, 0, err, &H,
                                  nullptr, &empty);
    if (st != MPQE_OK || empty) return st;
    if (!scores) return MPQE_ERR_INVALID_ARG;
    return gqe_fwd_mixed_launch<0>(H.G, desc, formula_of, num_queries, num_formulas, scores, stream);
}

// the rows the mixed forward would score, alone (intersection form): gqe_fwd_mixed_kernel's EMBED path, no E side
extern "C" int mpqe_gqe_embed_mixed(const int32_t *prog_host, int64_t num_formulas, const void *desc, size_t desc_bytes,
                                    const int64_t *node_map, int64_t node_map_len, int64_t dim, const int64_t *formula_of,
                                    int64_t num_queries, const int64_t *p_ids, float *out, int32_t *err, void *stream) {
    if (!prog_host || prog_host[0] != 1) return MPQE_ERR_INVALID_ARG;       // (chain form: by runs, mpqe_gqe_embed)
    GqeHost H;
    bool empty;
    // (one P row per query and no E rows: the sizes of the E side stand at the P side's, its ids are not read)
    const int st = gqe_mixed_call(prog_host, num_formulas, desc, desc_bytes, 0, 0, node_map, node_map_len, dim, formula_of,
                                  num_queries, p_ids, num_queries, p_ids, num_queries, nullptr, nullptr, num_queries, 0.f,
                                  nullptr, 0, err, &H, nullptr, &empty);
    if (st != MPQE_OK || empty) return st;
    if (!out || (uintptr_t)out % 16 != 0) return MPQE_ERR_INVALID_ARG;
    return gqe_fwd_mixed_launch<2>(H.G, desc, formula_of, num_queries, num_formulas, out, stream);
}

extern "C" int mpqe_gqe_fwd_mixed_save(const int32_t *prog_host, int64_t num_formulas, const void *desc, size_t desc_bytes,
                                       int num_tables, int num_mats, const int64_t *node_map, int64_t node_map_len,
                                       int64_t dim, const int64_t *formula_of, int64_t num_queries, const int64_t *p_ids,
                                       int64_t p_rows, const int64_t *e_ids, int64_t e_rows, const int64_t *qrow,
                                       const int64_t *neg_off, int64_t n, float eps, float *scores, void *workspace,
                                       size_t workspace_bytes, int32_t *err, void *stream) {
    GqeHost H;
    GqeMixLayout L;
    bool empty;
    const int st = gqe_mixed_call(prog_host, num_formulas, desc, desc_bytes, num_tables, num_mats, node_map, node_map_len, dim,
                                  formula_of, num_queries, p_ids, p_rows, e_ids, e_rows, qrow, neg_off, n, eps, workspace,
                                  workspace_bytes, err, &H, &L, &empty);
    if (st != MPQE_OK || empty) return st;
    if (!scores) return MPQE_ERR_INVALID_ARG;
    return gqe_fwd_mixed_launch<1>(H.G, desc, formula_of, num_queries, num_formulas, scores, stream);
}

extern "C" int mpqe_gqe_bwd_mixed(const int32_t *prog_host, int64_t num_formulas, const void *desc, size_t desc_bytes,
                                  const void *index, size_t index_bytes, int num_tables, int num_mats,
                                  const int64_t *node_map, int64_t node_map_len, int64_t dim, const int64_t *formula_of,
                                  int64_t num_queries, const int64_t *p_ids, int64_t p_rows, const int64_t *e_ids,
                                  int64_t e_rows, const int64_t *qrow, const int64_t *neg_off, int64_t n, float eps,
                                  const float *grad_scores, float *const *grad_tables_host, float *const *grad_mats_host,
                                  void *workspace, size_t workspace_bytes, int32_t *err, void *stream) {
    if (!grad_tables_host || (num_mats > 0 && !grad_mats_host)) return MPQE_ERR_INVALID_ARG;
    if (!index || (uintptr_t)index % 256 != 0) return MPQE_ERR_INVALID_ARG;
    if (num_formulas >= 1 && num_formulas < ((int64_t)1 << 24) && index_bytes < gqe_mixed_index_size(num_formulas))
        return MPQE_ERR_WORKSPACE;
    GqeHost H;
    GqeMixLayout L;
    bool empty;
    int st = gqe_mixed_call(prog_host, num_formulas, desc, desc_bytes, num_tables, num_mats, node_map, node_map_len, dim,
                            formula_of, num_queries, p_ids, p_rows, e_ids, e_rows, qrow, neg_off, n, eps, workspace,
                            workspace_bytes, err, &H, &L, &empty);
    if (st != MPQE_OK || empty) return st;
    if (!grad_scores) return MPQE_ERR_INVALID_ARG;
    GqeDev &G = H.G;
    GqeMixTrain &Tn = L.Tn;
    Tn.idx = reinterpret_cast<const GqeMixIdx *>(index);
    bool any_table = false, any_mat = false;
    hipStream_t s = as_stream(stream);
    char *wsb = reinterpret_cast<char *>(workspace);
    st = mix_upload_grad_ptrs(wsb + Tn.ptr_off * 4, (size_t)num_tables + (size_t)num_mats, s, [&](float **image) {
        for (int t = 0; t < num_tables; ++t) {
            image[t] = grad_tables_host[t];
            any_table = any_table || image[t];
        }
        for (int m = 0; m < num_mats; ++m) {
            image[num_tables + m] = grad_mats_host[m];
            any_mat = any_mat || image[num_tables + m];
        }
    });
    if (st != MPQE_OK) return st;
    // (every entry a stretch of a valid formula does not own: key -1)
    if (hipMemsetAsync(wsb + G.key_off * 4, 0xFF, (size_t)L.n_ent * 8, s) != hipSuccess) return MPQE_ERR_LAUNCH;
    const dim3 grid((unsigned)(G.Rp16 / GQ_ROWS * 16));
    if (G.dot)
        hipLaunchKernelGGL(gqe_bwd_mixed_kernel<1>, grid, dim3(256), 0, s, G, Tn, grad_scores);
    else
        hipLaunchKernelGGL(gqe_bwd_mixed_kernel<0>, grid, dim3(256), 0, s, G, Tn, grad_scores);
    st = mpqe_launch_status();
    if (st != MPQE_OK) return st;
    if (any_mat && Tn.NC > 0) {
        if (hipMemsetAsync(wsb + Tn.seg_off * 4, 0, (size_t)(num_mats + 1) * 8, s) != hipSuccess) return MPQE_ERR_LAUNCH;
        const dim3 cgrid((unsigned)((Tn.NC + 255) / 256));
        hipLaunchKernelGGL(gqe_mix_ckeys_kernel, cgrid, dim3(256), 0, s, G, Tn);
        int bits = 1;
        while ((1ll << bits) <= num_mats) ++bits;
        st = radix_sort_pairs_own<unsigned>(wsb + L.sort_off, reinterpret_cast<const unsigned *>(G.ws + Tn.ckey_off),
                                            reinterpret_cast<unsigned *>(G.ws + Tn.skey_off),
                                            reinterpret_cast<const int *>(G.ws + Tn.cval_off),
                                            reinterpret_cast<int *>(G.ws + Tn.sval_off), Tn.NC, bits, s);
        if (st != MPQE_OK) return st;
        hipLaunchKernelGGL(gqe_mix_seg_kernel, cgrid, dim3(256), 0, s, G, Tn);
        hipLaunchKernelGGL(gqe_mix_param_kernel, dim3((unsigned)((long long)num_mats * (G.D / 16))), dim3(256), 0, s, G, Tn);
        st = mpqe_launch_status();
        if (st != MPQE_OK) return st;
    }
    if (any_table) {
        hipLaunchKernelGGL(gqe_rows_mixed_kernel, dim3((unsigned)((L.n_ent + 3) / 4)), dim3(256), 0, s, G, Tn, L.n_ent);
        st = mpqe_launch_status();
    }
    return st;
}
