// The GQE baseline (reference model.py:57-134, decoders.py:123-150, 270-319) as one launch per formula batch.
//
// The host compiles a formula into a programme of MPQE_GQE_PROG_INTS ints (include/mpqe_amd.h): up to three branches,
// each a looked-up, L2-normalised embedding row taken through up to three [D, D] matrices; for two or three branches the
// intersection (optional pre matrix + ReLU, mean / min over the branches, optional post matrix); up to three more
// matrices; then the cosine against the rows of the other side. The rows that pass through the matrices are the
// "P side", the plain embedding rows they are scored against the "E side":
//   chain form   P rows = the n = B + sum(L) target / negative rows, E rows = the B anchors, pair r = (P r, E qrow[r])
//   inter form   P rows = the B queries, E rows = the n target / negative rows, pair r = (P of r's query, E r); the
//                negatives of query q are the rows B + neg_off[q] .. B + neg_off[q + 1] - 1
// As in step_chain.h a workgroup owns 16 P rows and keeps their states in LDS (three tiles: two ping-pong, one for the
// running aggregate / its gradient); a product is [16 rows] x [D] x [D] on v_mfma_f32_16x16x4_f32, lane l feeding
// A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], the matrix read straight from global memory in either
// orientation. One lane's four consecutive k (one 16-byte LDS read) feed four MFMAs, MFMA u multiplying
// k = 16 t + 4 (l >> 4) + u: the sum over k is re-ordered, in a fixed order.
//
// States the forward keeps for the backward (workspace, floats; Rp16 = P rows rounded up to 16):
//   X[site]   [Rp16, D]  the input rows of every matrix product (a site = one use of one matrix; at most 16)
//   T[b]      [Rp16, D]  the rows the aggregate is taken over (after the ReLU), per branch; only with >= 2 branches
//   Pfin      [Rp16, D]  the rows that are scored
// and the backward adds
//   dY[site]  [Rp16, D]  the gradient of every product's output
//   GE        [nb * Rp16 + n, D]  the gradient w.r.t. every looked-up, normalised row (branch sources, then E rows by pair)
//   key       [nb * Rp + n] int64  (table, row) of every looked-up row
// The state gradients are one launch (gqe_bwd_kernel). Matrix gradients are X^T . dY per site on the library's
// fixed-order weight-gradient tiles (mpqe_linear_bwd, added into the caller's buffer site after site in programme order:
// a matrix used at two sites gets both terms in that order). Entity-table rows: every looked-up row has one key; the
// first entry of a key sums the entries of that key in entry order and adds the sum to the table gradient (one writer
// per row, no float atomics: the same bits every run).
//
// Vector path operators (programme int [7]; reference decoders.py:181-236): with 1 (translate, TransE) or 2 (scale, the
// diagonal bilinear form) every branch and tail site owns a [D] vector, not a matrix, and is one elementwise pass over the
// tile in LDS, in place: x + v / x * v, site after site in programme order (three translations are ((x + v1) + v2) + v3).
// The pre / post products of the intersection stay matrices. Programme int [27] = 1 scores by the plain dot product
// (the diagonal decoder's chain form, decoders.py:228-233). Backward: translate passes dY on, scale gives dX = dY * v; a
// vector's gradient is the column sum over the p_rows real rows of dY (translate) / X * dY (scale): every workgroup of
// gqe_bwd_kernel adds its 16 rows in row order into one partial row per site, gqe_vec_final_kernel then adds the partial
// rows in a fixed order (four row groups per column, then the four sums in group order) and the sites in programme order
// into the caller's buffer: no float atomics, the same bits every run. Scale sites keep X; translate sites keep nothing,
// neither keeps a dY. (The padded rows of the last tile carry a gradient of exactly zero -- nothing is scored against
// them --, so leaving them out of the sum is a rule, not a correction.)
#include <string.h>

#include <new>

#include "mix_grad_core.h"

#define GQ_ROWS 16
#define GQ_MAXD 256
#define GQ_LDXMAX (GQ_MAXD + 4)
#define GQ_SITES 16
#define GQ_SITE_PRE 9
#define GQ_SITE_POST 12
#define GQ_SITE_TAIL 13
#define GQ_VEC_SITES 12       // branch and tail sites: the ones a vector operator can own

struct GqeDev {
    int form, nb, agg, ntail, has_pre, has_post, D, save;
    int op, dot;                   // path operator of the branch / tail sites (0 matrix, 1 translate, 2 scale); 1: dot scoring
    int bn[3], bT[3][3], tT[3];
    const float *tab[4];           // tables of the branch sources, then of the E side
    float *gtab[4];                // their gradients (backward; NULL = not wanted)
    long long tab_rows[4];
    int tmode[4];
    const float *w[GQ_SITES];
    long long x_off[GQ_SITES], dy_off[GQ_SITES];
    long long t_off[3], pfin_off, ge_off, key_off;
    long long part_off[GQ_SITES];  // vector sites: [Rp16 / 16, D] partial column sums of the site's vector gradient
    const long long *node_map;
    long long map_len;
    const long long *p_ids, *e_ids, *qrow, *neg_off;
    long long Rp, Rp16, Re, n;
    float eps;
    float *ws;
    int32_t *err;
};

// one table row, L2-normalised, 4 floats per lane (lanes with 4 * lane >= D hold zeros): the arithmetic of row_norm_store
__device__ __forceinline__ f32x4 gq_norm_row(const float *tab, long long row, int D, int lane) {
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
    const int c = lane * 4;
    if (row >= 0 && c < D) q = gload4(tab + row * D + c);
    const float ss = wave_sum(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float nrm = sqrtf(ss);
    if (row >= 0) {
        q[0] /= nrm; q[1] /= nrm; q[2] /= nrm; q[3] /= nrm;
    }
    return q;
}

// rows [i0, i0 + 16) of one id list -> tile (rows past `R` and bad ids: zeros); ids == NULL: row r of the table itself
__device__ __forceinline__ void gq_gather(const GqeDev &G, float *tile, int LDX, const long long *ids, int slot, long long i0,
                                          long long R) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < GQ_ROWS; i += 4) {
        const long long r = i0 + i;
        long long row = -1;
        if (r < R) row = ids ? lookup_row(G.node_map, G.map_len, ids[r], G.tab_rows[slot], lane == 0 ? G.err : nullptr) : r;
        const f32x4 q = gq_norm_row(G.tab[slot], row, G.D, lane);
        if (lane * 4 < G.D) *reinterpret_cast<f32x4 *>(tile + i * LDX + lane * 4) = q;
    }
}

// dst = [relu](src . M) (T = 0) or src . M^T (T = 1), M [D, D] row-major in global memory
__device__ __forceinline__ void gq_mm(const float *src, float *dst, const float *W, int D, int LDX, int T, int relu) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, kq = lane >> 4;
    for (int cb = wave; cb < D / 16; cb += 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int col = cb * 16 + j;
        for (int t = 0; t < D / 16; ++t) {
            const int k0 = 16 * t + 4 * kq;
            const f32x4 a = *reinterpret_cast<const f32x4 *>(src + j * LDX + k0);
            f32x4 b;
            if (T) {
                b = gload4(W + (long long)col * D + k0);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) b[u] = gload1(W + (long long)(k0 + u) * D + col);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc[r];
            if (relu) v = v > 0.f ? v : 0.f;
            dst[(4 * kq + r) * LDX + col] = v;
        }
    }
}

// one vector site, in place: x + v (op 1) / x * v (op 2). Lane l holds v[4 l .. 4 l + 3] (one 16-byte global read per
// wave), wave w walks rows w, w + 4, ... xsave != NULL: the input rows go to rows [i0, i0 + 16) of that [Rp16, D] state
// first, from the thread that then changes them (the pass is in place: a separate gq_store would race with it).
__device__ __forceinline__ void gq_vec(float *tile, int LDX, const float *v, int D, int op, float *xsave, long long i0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane * 4;
    if (c >= D) return;
    const f32x4 w = gload4(v + c);
    for (int i = wave; i < GQ_ROWS; i += 4) {
        f32x4 x = *reinterpret_cast<const f32x4 *>(tile + i * LDX + c);
        if (xsave) *reinterpret_cast<f32x4 *>(xsave + (i0 + i) * D + c) = x;
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = op == 1 ? x[u] + w[u] : x[u] * w[u];
        *reinterpret_cast<f32x4 *>(tile + i * LDX + c) = x;
    }
}

// the backward of one vector site on the tile of dY, in place: the workgroup's partial row of the vector's gradient (the
// rows below Rp, in row order: padded rows hold no query) -> part; scale: dX = dY * v. Thread t < D / 4 owns 4 columns.
__device__ __forceinline__ void gq_vec_bwd(float *tile, int LDX, const float *v, const float *X, float *part, long long i0,
                                           long long Rp, int D, int op) {
    const int c = threadIdx.x * 4;
    if (c >= D) return;
    f32x4 w = {1.f, 1.f, 1.f, 1.f}, s = {0.f, 0.f, 0.f, 0.f};
    if (op == 2) w = gload4(v + c);
    for (int i = 0; i < GQ_ROWS; ++i) {
        f32x4 g = *reinterpret_cast<const f32x4 *>(tile + i * LDX + c);
        if (i0 + i < Rp) {
            if (op == 2) {
                const f32x4 x = gload4(X + (i0 + i) * D + c);
#pragma unroll
                for (int u = 0; u < 4; ++u) s[u] += x[u] * g[u];
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) s[u] += g[u];
            }
        }
        if (op == 2) {
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] *= w[u];
            *reinterpret_cast<f32x4 *>(tile + i * LDX + c) = g;
        }
    }
    *reinterpret_cast<f32x4 *>(part + (i0 / GQ_ROWS) * D + c) = s;
}

// tile -> rows [i0, i0 + 16) of a [Rp16, D] state
__device__ __forceinline__ void gq_store(const float *tile, int LDX, float *g, long long i0, int D) {
    const int per = D / 4;
    for (int e = threadIdx.x; e < GQ_ROWS * per; e += 256) {
        const int i = e / per, c = (e % per) * 4;
        *reinterpret_cast<f32x4 *>(g + (i0 + i) * D + c) = *reinterpret_cast<const f32x4 *>(tile + i * LDX + c);
    }
}
__device__ __forceinline__ void gq_load(float *tile, int LDX, const float *g, long long i0, int D) {
    const int per = D / 4;
    for (int e = threadIdx.x; e < GQ_ROWS * per; e += 256) {
        const int i = e / per, c = (e % per) * 4;
        *reinterpret_cast<f32x4 *>(tile + i * LDX + c) = gload4(g + (i0 + i) * D + c);
    }
}

// the E row of pair r, normalised (zeros for a bad id / a bad row map entry)
__device__ __forceinline__ f32x4 gq_e_row(const GqeDev &G, long long r, int lane) {
    long long row = -1;
    if (r < G.n) {
        long long e = r;
        if (G.form == 0) {
            e = G.qrow[r];
            if (e < 0 || e >= G.Re) {
                if (lane == 0) flag_error(G.err, MPQE_FLAG_BAD_INDEX);
                e = -1;
            }
        }
        if (e >= 0) row = lookup_row(G.node_map, G.map_len, G.e_ids[e], G.tab_rows[3], lane == 0 ? G.err : nullptr);
    }
    return gq_norm_row(G.tab[3], row, G.D, lane);
}

// the negatives of query q: rows [lo, hi) of the pair list
__device__ __forceinline__ void gq_neg_range(const GqeDev &G, long long q, int lane, long long &lo, long long &hi) {
    lo = hi = 0;
    const long long nneg = G.n - G.Rp;
    if (!G.neg_off || q >= G.Rp) return;
    long long a = G.neg_off[q], b = G.neg_off[q + 1];
    if (a < 0 || b < a || b > nneg) {
        if (lane == 0) flag_error(G.err, MPQE_FLAG_BAD_INDEX);
        a = a < 0 ? 0 : (a > nneg ? nneg : a);
        b = b < a ? a : (b > nneg ? nneg : b);
    }
    lo = G.Rp + a;
    hi = G.Rp + b;
}

// the score of (p, e) by mpqe_cosine_fwd's definition; with g != NULL also the two gradients
__device__ __forceinline__ float gq_cos(const f32x4 p, const f32x4 e, float eps, const float *g, f32x4 *gp, f32x4 *ge) {
    const float dot = wave_sum(p[0] * e[0] + p[1] * e[1] + p[2] * e[2] + p[3] * e[3]);
    const float qq = wave_sum(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]);
    const float tt = wave_sum(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3]);
    const float rq = sqrtf(qq), rt = sqrtf(tt);
    const float nq = fmaxf(rq, eps), nt = fmaxf(rt, eps);
    if (!g) return dot / (nq * nt);
    const float inv = 1.f / (nq * nt);
    const float s = dot * inv;
    const float kq = rq > eps ? s / (nq * nq) : 0.f;
    const float kt = rt > eps ? s / (nt * nt) : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        (*gp)[u] = *g * (e[u] * inv - kq * p[u]);
        (*ge)[u] = *g * (p[u] * inv - kt * e[u]);
    }
    return s;
}

// the plain dot product (decoders.py:232); with g != NULL also the two gradients
__device__ __forceinline__ float gq_dot(const f32x4 p, const f32x4 e, const float *g, f32x4 *gp, f32x4 *ge) {
    const float dot = wave_sum(p[0] * e[0] + p[1] * e[1] + p[2] * e[2] + p[3] * e[3]);
    if (g) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            (*gp)[u] = *g * e[u];
            (*ge)[u] = *g * p[u];
        }
    }
    return dot;
}
// (the score is a template parameter of the kernels, not a branch: the cosine instantiation's scoring code is the one it
// was before the dot score existed, and gives the same bits)
template <int DOT>
__device__ __forceinline__ float gq_score(const GqeDev &G, const f32x4 p, const f32x4 e, const float *g, f32x4 *gp,
                                          f32x4 *ge) {
    if (DOT) return gq_dot(p, e, g, gp, ge);
    return gq_cos(p, e, G.eps, g, gp, ge);
}

// EMBED = 0: the forward. EMBED = 1 (mpqe_gqe_embed): the same P side, then the rows the forward would score go to
// `scores` as [Rp, D] -- no E side, no states; G.p_ids == NULL (one branch): P row r is row r of the branch's table.
// DOT = 1: the pairs are scored by the plain dot product.
template <int EMBED, int DOT>
__global__ __launch_bounds__(256) void gqe_fwd_kernel(GqeDev G, float *__restrict__ scores) {
    __shared__ __attribute__((aligned(16))) float lds[3 * GQ_ROWS * GQ_LDXMAX];
    const int D = G.D, LDX = D + 4, per = D / 4;
    const bool save = !EMBED && G.save;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i0 = (long long)blockIdx.x * GQ_ROWS;
    float *cur = lds, *nxt = lds + GQ_ROWS * LDX, *agg = lds + 2 * GQ_ROWS * LDX;

    for (int b = 0; b < G.nb; ++b) {
        gq_gather(G, cur, LDX, G.p_ids ? G.p_ids + (long long)b * G.Rp : nullptr, b, i0, G.Rp);
        __syncthreads();
        for (int s = 0; s < G.bn[b]; ++s) {
            const int site = 3 * b + s;
            if (G.op) {
                gq_vec(cur, LDX, G.w[site], D, G.op, save && G.op == 2 ? G.ws + G.x_off[site] : nullptr, i0);
                __syncthreads();
                continue;
            }
            if (save) gq_store(cur, LDX, G.ws + G.x_off[site], i0, D);
            gq_mm(cur, nxt, G.w[site], D, LDX, G.bT[b][s], 0);
            __syncthreads();
            float *t = cur; cur = nxt; nxt = t;
        }
        if (G.nb < 2) break;
        if (G.has_pre) {
            if (save) gq_store(cur, LDX, G.ws + G.x_off[GQ_SITE_PRE + b], i0, D);
            gq_mm(cur, nxt, G.w[GQ_SITE_PRE + b], D, LDX, 1, 1);
            __syncthreads();
            float *t = cur; cur = nxt; nxt = t;
        }
        if (save) gq_store(cur, LDX, G.ws + G.t_off[b], i0, D);
        for (int e = threadIdx.x; e < GQ_ROWS * per; e += 256) {
            const int o = (e / per) * LDX + (e % per) * 4;
            f32x4 v = *reinterpret_cast<const f32x4 *>(cur + o);
            if (b > 0) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(agg + o);
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = G.agg ? (v[u] < a[u] ? v[u] : a[u]) : a[u] + v[u];
            }
            if (!G.agg && b == G.nb - 1) {
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] /= (float)G.nb;
            }
            *reinterpret_cast<f32x4 *>(agg + o) = v;
        }
        __syncthreads();
    }
    if (G.nb >= 2) {
        // (the aggregate becomes the current tile; the two others are free)
        float *t = cur; cur = agg; agg = t;
        if (G.has_post) {
            if (save) gq_store(cur, LDX, G.ws + G.x_off[GQ_SITE_POST], i0, D);
            gq_mm(cur, nxt, G.w[GQ_SITE_POST], D, LDX, 1, 0);
            __syncthreads();
            t = cur; cur = nxt; nxt = t;
        }
    }
    for (int s = 0; s < G.ntail; ++s) {
        const int site = GQ_SITE_TAIL + s;
        if (G.op) {
            gq_vec(cur, LDX, G.w[site], D, G.op, save && G.op == 2 ? G.ws + G.x_off[site] : nullptr, i0);
            __syncthreads();
            continue;
        }
        if (save) gq_store(cur, LDX, G.ws + G.x_off[site], i0, D);
        gq_mm(cur, nxt, G.w[site], D, LDX, G.tT[s], 0);
        __syncthreads();
        float *t = cur; cur = nxt; nxt = t;
    }
    if (save) gq_store(cur, LDX, G.ws + G.pfin_off, i0, D);
    if (EMBED) {
        // (the tail tile: rows past Rp are not stored)
        for (int e = threadIdx.x; e < GQ_ROWS * per; e += 256) {
            const int i = e / per, c = (e % per) * 4;
            if (i0 + i < G.Rp)
                *reinterpret_cast<f32x4 *>(scores + (i0 + i) * D + c) = *reinterpret_cast<const f32x4 *>(cur + i * LDX + c);
        }
        return;
    }

    for (int i = wave; i < GQ_ROWS; i += 4) {
        const long long q = i0 + i;
        f32x4 p = {0.f, 0.f, 0.f, 0.f};
        if (lane * 4 < D) p = *reinterpret_cast<const f32x4 *>(cur + i * LDX + lane * 4);
        if (G.form == 0) {
            if (q < G.n) {
                const float s = gq_score<DOT>(G, p, gq_e_row(G, q, lane), nullptr, nullptr, nullptr);
                if (lane == 0) scores[q] = s;
            }
        } else if (q < G.Rp) {
            long long lo, hi;
            gq_neg_range(G, q, lane, lo, hi);
            for (long long r = q;;) {
                const float s = gq_score<DOT>(G, p, gq_e_row(G, r, lane), nullptr, nullptr, nullptr);
                if (lane == 0) scores[r] = s;
                r = r == q ? lo : r + 1;
                if (r >= hi) break;
            }
        }
    }
}

template <int DOT>
__global__ __launch_bounds__(256) void gqe_bwd_kernel(GqeDev G, const float *__restrict__ gs) {
    __shared__ __attribute__((aligned(16))) float lds[3 * GQ_ROWS * GQ_LDXMAX];
    const int D = G.D, LDX = D + 4, per = D / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i0 = (long long)blockIdx.x * GQ_ROWS;
    float *cur = lds, *nxt = lds + GQ_ROWS * LDX, *ga = lds + 2 * GQ_ROWS * LDX;
    float *GE = G.ws + G.ge_off;
    const long long ge_e0 = (long long)G.nb * G.Rp16;      // first E entry row of GE

    // scores: the gradient of the scored rows -> cur, of the E rows -> GE
    for (int i = wave; i < GQ_ROWS; i += 4) {
        const long long q = i0 + i;
        f32x4 p = {0.f, 0.f, 0.f, 0.f}, gp = {0.f, 0.f, 0.f, 0.f};
        if (lane * 4 < D) p = gload4(G.ws + G.pfin_off + q * D + lane * 4);
        if (G.form == 0) {
            if (q < G.n) {
                f32x4 ge;
                const float g = gs[q];
                gq_score<DOT>(G, p, gq_e_row(G, q, lane), &g, &gp, &ge);
                if (lane * 4 < D) *reinterpret_cast<f32x4 *>(GE + (ge_e0 + q) * D + lane * 4) = ge;
            }
        } else if (q < G.Rp) {
            long long lo, hi;
            gq_neg_range(G, q, lane, lo, hi);
            for (long long r = q;;) {
                f32x4 g1, ge;
                const float g = gs[r];
                gq_score<DOT>(G, p, gq_e_row(G, r, lane), &g, &g1, &ge);
#pragma unroll
                for (int u = 0; u < 4; ++u) gp[u] += g1[u];
                if (lane * 4 < D) *reinterpret_cast<f32x4 *>(GE + (ge_e0 + r) * D + lane * 4) = ge;
                r = r == q ? lo : r + 1;
                if (r >= hi) break;
            }
        }
        if (lane * 4 < D) *reinterpret_cast<f32x4 *>(cur + i * LDX + lane * 4) = gp;
    }
    __syncthreads();

    for (int s = G.ntail - 1; s >= 0; --s) {
        const int site = GQ_SITE_TAIL + s;
        if (G.op) {
            gq_vec_bwd(cur, LDX, G.w[site], G.ws + G.x_off[site], G.ws + G.part_off[site], i0, G.Rp, D, G.op);
            __syncthreads();
            continue;
        }
        gq_store(cur, LDX, G.ws + G.dy_off[site], i0, D);
        gq_mm(cur, nxt, G.w[site], D, LDX, !G.tT[s], 0);
        __syncthreads();
        float *t = cur; cur = nxt; nxt = t;
    }
    if (G.nb >= 2) {
        if (G.has_post) {
            gq_store(cur, LDX, G.ws + G.dy_off[GQ_SITE_POST], i0, D);
            gq_mm(cur, nxt, G.w[GQ_SITE_POST], D, LDX, 0, 0);
            __syncthreads();
            float *t = cur; cur = nxt; nxt = t;
        }
        float *t = cur; cur = ga; ga = t;       // ga: the gradient of the aggregate, kept over the branches
    }
    for (int b = 0; b < G.nb; ++b) {
        if (G.nb >= 2) {
            for (int e = threadIdx.x; e < GQ_ROWS * per; e += 256) {
                const int i = e / per, c = (e % per) * 4;
                const f32x4 g = *reinterpret_cast<const f32x4 *>(ga + i * LDX + c);
                f32x4 tv[3];
                for (int k = 0; k < G.nb; ++k) tv[k] = gload4(G.ws + G.t_off[k] + (i0 + i) * D + c);
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
                gq_store(cur, LDX, G.ws + G.dy_off[GQ_SITE_PRE + b], i0, D);
                gq_mm(cur, nxt, G.w[GQ_SITE_PRE + b], D, LDX, 0, 0);
                __syncthreads();
                float *t = cur; cur = nxt; nxt = t;
            }
        }
        for (int s = G.bn[b] - 1; s >= 0; --s) {
            const int site = 3 * b + s;
            if (G.op) {
                gq_vec_bwd(cur, LDX, G.w[site], G.ws + G.x_off[site], G.ws + G.part_off[site], i0, G.Rp, D, G.op);
                __syncthreads();
                continue;
            }
            gq_store(cur, LDX, G.ws + G.dy_off[site], i0, D);
            gq_mm(cur, nxt, G.w[site], D, LDX, !G.bT[b][s], 0);
            __syncthreads();
            float *t = cur; cur = nxt; nxt = t;
        }
        gq_store(cur, LDX, GE + (long long)b * G.Rp16 * D, i0, D);
        __syncthreads();
    }
}

// entry e of the looked-up rows: branch sources (b, i) in branch order, then the E row of every pair
__device__ __forceinline__ void gq_entry(const GqeDev &G, long long e, int &slot, long long &id_pos, long long &ge_row) {
    const long long np = (long long)G.nb * G.Rp;
    if (e < np) {
        slot = (int)(e / G.Rp);
        id_pos = e;
        ge_row = (long long)slot * G.Rp16 + e % G.Rp;
    } else {
        slot = 3;
        id_pos = e - np;
        ge_row = (long long)G.nb * G.Rp16 + (e - np);
    }
}

__global__ __launch_bounds__(256) void gqe_keys_kernel(GqeDev G, long long n_ent) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ent) return;
    int slot;
    long long pos, ge_row;
    gq_entry(G, e, slot, pos, ge_row);
    long long key = -1;
    if (G.gtab[slot]) {
        long long id = -1;
        bool ok = true;
        if (slot < 3) id = G.p_ids[pos];
        else if (G.form == 0) {
            const long long q = G.qrow[pos];
            ok = q >= 0 && q < G.Re;
            if (ok) id = G.e_ids[q];
        } else id = G.e_ids[pos];
        if (ok) {
            const long long row = lookup_row(G.node_map, G.map_len, id, G.tab_rows[slot], nullptr);     // (flagged by the forward)
            if (row >= 0) key = ((long long)G.tmode[slot] << 40) | row;
        }
    }
    reinterpret_cast<long long *>(G.ws + G.key_off)[e] = key;
}

// rows_reduce's entries (mix_grad_core.h): keys and GE rows in the workspace, the table and its gradient by the entry's slot
struct GqeEntries {
    const GqeDev &G;
    __device__ __forceinline__ const long long *keys() const { return reinterpret_cast<const long long *>(G.ws + G.key_off); }
    __device__ __forceinline__ void tables(long long e, long long, const float *&tab, float *&gtab) const {
        int slot;
        long long pos, ger;
        gq_entry(G, e, slot, pos, ger);
        tab = G.tab[slot];
        gtab = G.gtab[slot];
    }
    __device__ __forceinline__ const float *grad_row(long long e) const {
        int slot;
        long long pos, ger;
        gq_entry(G, e, slot, pos, ger);
        return G.ws + G.ge_off + ger * G.D;
    }
};

__global__ __launch_bounds__(256) void gqe_rows_kernel(GqeDev G, long long n_ent) { rows_reduce(GqeEntries{G}, n_ent, G.D); }

// The vector gradients from the workgroups' partial rows (gq_vec_bwd), the house form of bias_grad.h: one workgroup,
// thread = (row group rg of 4, column); a row group adds every 4th partial row in order (eight loads in flight), the four
// sums are added in group order, and the sites follow each other in programme order in the same thread -- a vector used at
// two sites gets both terms in that order. A fixed order: the same bits every run.
struct GqeVecFin {
    const float *part[GQ_VEC_SITES];
    float *grad[GQ_VEC_SITES];
    int n;
};

__global__ __launch_bounds__(4 * GQ_MAXD) void gqe_vec_final_kernel(GqeVecFin F, long long nblk, int D) {
    __shared__ float sums[4][GQ_MAXD];
    const int col = threadIdx.x % GQ_MAXD, rg = threadIdx.x / GQ_MAXD;
    for (int k = 0; k < F.n; ++k) {
        float s = 0.f;
        if (col < D)
            for (long long b0 = rg; b0 < nblk; b0 += 4 * 8) {
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const long long b = b0 + 4 * q;
                    v[q] = F.part[k][(b < nblk ? b : b0) * D + col];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (b0 + 4 * q < nblk) s += v[q];
            }
        sums[rg][col] = s;
        __syncthreads();
        if (rg == 0 && col < D) F.grad[k][col] += ((sums[0][col] + sums[1][col]) + sums[2][col]) + sums[3][col];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct GqeHost {
    GqeDev G;
    int site_mat[GQ_SITES];       // matrix index of every site, -1 = unused
    int site_T[GQ_SITES];
    size_t lin_off, lin_bytes, total;
};

// whether site s holds a [D] vector under path operator op: the branch and tail sites do, the pre / post products never
static bool gqe_vec_site(int op, int s) {
    return op != 0 && (s < GQ_SITE_PRE || s >= GQ_SITE_TAIL);
}

static int gqe_step(int code, int num_mats, int *mat, int *T) {
    if (code < 0) return 1;
    *mat = code >> 1;
    *T = code & 1;
    return num_mats >= 0 && *mat >= num_mats;
}

// programme + sizes -> device record and workspace layout; num_mats < 0: the sizes only (no bound on matrix indices)
static int gqe_plan(const int32_t *prog, int num_tables, int num_mats, int64_t dim, int64_t p_rows, int64_t e_rows, int64_t n,
                    GqeHost *H) {
    if (!prog || p_rows < 1 || n < 1 || dim <= 0) return MPQE_ERR_INVALID_ARG;
    if (dim % 16 != 0 || dim > GQ_MAXD) return MPQE_ERR_UNSUPPORTED;
    if (p_rows >= (1ll << 31) || n >= (1ll << 31)) return MPQE_ERR_UNSUPPORTED;
    memset(H, 0, sizeof(*H));
    GqeDev &G = H->G;
    G.form = prog[0];
    G.nb = prog[1];
    G.agg = prog[2];
    G.ntail = prog[5];
    G.D = (int)dim;
    if (G.form < 0 || G.form > 1 || G.nb < 1 || G.nb > 3 || G.agg < 0 || G.agg > 1 || G.ntail < 0 || G.ntail > 3)
        return MPQE_ERR_INVALID_ARG;
    // ([27] = -1 is what programmes written before the dot score existed carry there: the cosine)
    if (prog[7] < 0 || prog[7] > 2 || prog[27] < -1 || prog[27] > 1) return MPQE_ERR_INVALID_ARG;
    G.op = prog[7];
    G.dot = prog[27] == 1;
    if (G.form == 0 ? (p_rows != n || e_rows < 1) : (e_rows != n || n < p_rows)) return MPQE_ERR_INVALID_ARG;
    if (G.nb == 1 && (prog[3] >= 0 || prog[4] >= 0)) return MPQE_ERR_INVALID_ARG;
    for (int s = 0; s < GQ_SITES; ++s) H->site_mat[s] = -1;
    for (int t = 0; t < 4; ++t) {
        const int mode = t < 3 ? (t < G.nb ? prog[8 + 5 * t] : 0) : prog[6];
        if (num_tables >= 0 && (mode < 0 || mode >= num_tables)) return MPQE_ERR_INVALID_ARG;
        G.tmode[t] = mode;
    }
    for (int b = 0; b < G.nb; ++b) {
        G.bn[b] = prog[9 + 5 * b];
        if (G.bn[b] < 0 || G.bn[b] > 3) return MPQE_ERR_INVALID_ARG;
        for (int s = 0; s < G.bn[b]; ++s) {
            if (gqe_step(prog[10 + 5 * b + s], num_mats, &H->site_mat[3 * b + s], &H->site_T[3 * b + s])) return MPQE_ERR_INVALID_ARG;
            G.bT[b][s] = H->site_T[3 * b + s];
        }
    }
    if (G.nb >= 2) {
        if (prog[3] >= 0) {
            if (num_mats >= 0 && prog[3] >= num_mats) return MPQE_ERR_INVALID_ARG;
            G.has_pre = 1;
            for (int b = 0; b < G.nb; ++b) {
                H->site_mat[GQ_SITE_PRE + b] = prog[3];
                H->site_T[GQ_SITE_PRE + b] = 1;
            }
        }
        if (prog[4] >= 0) {
            if (num_mats >= 0 && prog[4] >= num_mats) return MPQE_ERR_INVALID_ARG;
            G.has_post = 1;
            H->site_mat[GQ_SITE_POST] = prog[4];
            H->site_T[GQ_SITE_POST] = 1;
        }
    }
    for (int s = 0; s < G.ntail; ++s) {
        if (gqe_step(prog[24 + s], num_mats, &H->site_mat[GQ_SITE_TAIL + s], &H->site_T[GQ_SITE_TAIL + s])) return MPQE_ERR_INVALID_ARG;
        G.tT[s] = H->site_T[GQ_SITE_TAIL + s];
    }
    G.Rp = p_rows;
    G.Rp16 = (p_rows + 15) / 16 * 16;
    G.Re = e_rows;
    G.n = n;
    // workspace (floats; every block a multiple of 64 floats = 256 bytes)
    const long long blk = G.Rp16 * dim;
    long long off = 0;
    for (int s = 0; s < GQ_SITES; ++s) {
        G.x_off[s] = G.dy_off[s] = G.part_off[s] = -1;
        if (H->site_mat[s] < 0) continue;
        if (gqe_vec_site(G.op, s)) {
            // (a vector site: X only where the gradient reads it, and one partial row per workgroup)
            if (G.op == 2) {
                G.x_off[s] = off;
                off += blk;
            }
            G.part_off[s] = off;
            off += (long long)align_up((size_t)(G.Rp16 / GQ_ROWS) * (size_t)dim, 64);
            continue;
        }
        G.x_off[s] = off;
        G.dy_off[s] = off + blk;
        off += 2 * blk;
    }
    for (int b = 0; b < 3; ++b) {
        G.t_off[b] = -1;
        if (G.nb >= 2 && b < G.nb) {
            G.t_off[b] = off;
            off += blk;
        }
    }
    G.pfin_off = off;
    off += blk;
    G.ge_off = off;
    off += (long long)align_up((size_t)((long long)G.nb * G.Rp16 + n) * (size_t)dim, 64);
    G.key_off = off;
    off += (long long)align_up((size_t)((long long)G.nb * p_rows + n) * 2, 64);
    H->lin_off = (size_t)off * 4;
    H->lin_bytes = mpqe_linear_bwd_workspace_bytes(p_rows, dim, dim);
    H->total = H->lin_off + H->lin_bytes + 256;
    return MPQE_OK;
}

extern "C" size_t mpqe_gqe_workspace_bytes(const int32_t *prog_host, int64_t p_rows, int64_t n, int64_t dim) {
    GqeHost H;
    if (!prog_host) return 0;
    const int64_t e_rows = prog_host[0] == 0 ? 1 : n;
    if (gqe_plan(prog_host, -1, -1, dim, p_rows, e_rows, n, &H) != MPQE_OK) return 0;
    return H.total;
}

static int gqe_bind(GqeHost *H, const float *const *tables, const int64_t *table_rows, const int64_t *node_map,
                    int64_t node_map_len, const float *const *mats, const int64_t *p_ids, const int64_t *e_ids,
                    const int64_t *qrow, const int64_t *neg_off, float eps, void *workspace, int32_t *err,
                    bool p_only = false) {
    GqeDev &G = H->G;
    if (!tables || !table_rows || !mats || node_map_len < 0) return MPQE_ERR_INVALID_ARG;
    if (!p_only) {
        if (!p_ids || !e_ids) return MPQE_ERR_INVALID_ARG;
        if (G.form == 0 && !qrow) return MPQE_ERR_INVALID_ARG;
        if (G.form == 1 && G.n > G.Rp && !neg_off) return MPQE_ERR_INVALID_ARG;
    }
    for (int t = 0; t < (p_only ? 3 : 4); ++t) {
        if (t < 3 && t >= G.nb) continue;
        G.tab[t] = tables[G.tmode[t]];
        G.tab_rows[t] = table_rows[G.tmode[t]];
        if (!G.tab[t] || G.tab_rows[t] < 0 || (uintptr_t)G.tab[t] % 16 != 0) return MPQE_ERR_INVALID_ARG;
    }
    for (int s = 0; s < GQ_SITES; ++s) {
        if (H->site_mat[s] < 0) continue;
        G.w[s] = mats[H->site_mat[s]];
        if (!G.w[s] || (uintptr_t)G.w[s] % 16 != 0) return MPQE_ERR_INVALID_ARG;
    }
    G.node_map = (const long long *)node_map;
    G.map_len = node_map_len;
    G.p_ids = (const long long *)p_ids;
    G.e_ids = (const long long *)e_ids;
    G.qrow = (const long long *)qrow;
    G.neg_off = (const long long *)neg_off;
    G.eps = eps;
    G.ws = reinterpret_cast<float *>(workspace);
    G.err = err;
    return MPQE_OK;
}

extern "C" int mpqe_gqe_fwd(const int32_t *prog_host, const float *const *tables_host, const int64_t *table_rows_host,
                            int num_tables, const int64_t *node_map, int64_t node_map_len, const float *const *mats_host,
                            int num_mats, int64_t dim, const int64_t *p_ids, int64_t p_rows, const int64_t *e_ids,
                            int64_t e_rows, const int64_t *qrow, const int64_t *neg_off, int64_t n, float eps, int save_states,
                            float *scores, void *workspace, size_t workspace_bytes, int32_t *err, void *stream) {
    if (num_tables < 1 || num_mats < 0 || !scores) return MPQE_ERR_INVALID_ARG;
    GqeHost H;
    int st = gqe_plan(prog_host, num_tables, num_mats, dim, p_rows, e_rows, n, &H);
    if (st != MPQE_OK) return st;
    st = gqe_bind(&H, tables_host, table_rows_host, node_map, node_map_len, mats_host, p_ids, e_ids, qrow, neg_off, eps,
                  workspace, err);
    if (st != MPQE_OK) return st;
    H.G.save = save_states != 0;
    if (H.G.save) {
        if (!workspace || (uintptr_t)workspace % 256 != 0) return MPQE_ERR_INVALID_ARG;
        if (workspace_bytes < H.total) return MPQE_ERR_WORKSPACE;
    }
    if (H.G.dot)
        hipLaunchKernelGGL((gqe_fwd_kernel<0, 1>), dim3((unsigned)(H.G.Rp16 / GQ_ROWS)), dim3(256), 0, as_stream(stream), H.G,
                           scores);
    else
        hipLaunchKernelGGL((gqe_fwd_kernel<0, 0>), dim3((unsigned)(H.G.Rp16 / GQ_ROWS)), dim3(256), 0, as_stream(stream), H.G,
                           scores);
    return mpqe_launch_status();
}

// the rows a programme scores, alone: the forward's P side with EMBED = 1 (no E side: the programme's [6] is not read)
extern "C" int mpqe_gqe_embed(const int32_t *prog_host, const float *const *tables_host, const int64_t *table_rows_host,
                              int num_tables, const int64_t *node_map, int64_t node_map_len, const float *const *mats_host,
                              int num_mats, int64_t dim, const int64_t *p_ids, int64_t p_rows, float *out, int32_t *err,
                              void *stream) {
    if (num_tables < 1 || num_mats < 0 || !out || !prog_host) return MPQE_ERR_INVALID_ARG;
    int32_t prog[MPQE_GQE_PROG_INTS];
    memcpy(prog, prog_host, sizeof(prog));
    prog[6] = prog[8];                  // (the plan checks an E table: branch 0's, which it checks anyway)
    GqeHost H;
    int st = gqe_plan(prog, num_tables, num_mats, dim, p_rows, p_rows, p_rows, &H);
    if (st != MPQE_OK) return st;
    st = gqe_bind(&H, tables_host, table_rows_host, p_ids ? node_map : nullptr, node_map_len, mats_host, p_ids, nullptr,
                  nullptr, nullptr, 0.f, nullptr, err, true);
    if (st != MPQE_OK) return st;
    if ((uintptr_t)out % 16 != 0) return MPQE_ERR_INVALID_ARG;
    if (!p_ids && (H.G.nb != 1 || p_rows > H.G.tab_rows[0])) return MPQE_ERR_INVALID_ARG;
    hipLaunchKernelGGL((gqe_fwd_kernel<1, 0>), dim3((unsigned)(H.G.Rp16 / GQ_ROWS)), dim3(256), 0, as_stream(stream), H.G, out);
    return mpqe_launch_status();
}

// ------------------------------------------------------------------------------- queries of different formulas at once
// mpqe_gqe_fwd_mixed: the forward without states for B queries of ONE query type, query q under programme formula_of[q]
// of F. The programmes share what the query type fixes (form, branches, products per branch and after the merge, operator,
// scoring, aggregate, pre / post presence); a formula's own part -- its tables, the parameter and transposition of every
// site -- is one GqeMixDesc in device memory (mpqe_gqe_mixed_desc_build; it depends on the programmes and the parameter
// addresses only, so the caller keeps the block between calls).
// Tiles without a tile table: the P rows (intersection form: the B queries; chain form: the n pair rows, row r belonging
// to query qrow[r]) are cut into blocks of 16, and a block into its maximal stretches of rows with one formula; workgroup
// 16 k + j owns the j-th stretch of block k and leaves at once when the block has fewer. Every workgroup reads the block's
// (at most 16) formula indices with uniform loads, so there is no pre-pass, no workspace and one launch. A stretch is a
// tile of gqe_fwd_kernel with fewer rows: the shared helpers run on a GqeDev put together from the shared record and the
// stretch's descriptor, every output element's sum over k has gq_mm's fixed order whichever tile row it sits in, and the
// scores are mpqe_gqe_fwd's to the bit. A formula index outside [0, F) (chain form also: a qrow outside [0, B)) flags
// MPQE_FLAG_BAD_INDEX and its rows score 0.
struct GqeMixDesc {
    const float *tab[4];
    long long tab_rows[4];
    const float *w[GQ_SITES];
    int T[GQ_SITES];
};

// the formula of P row r, -1 for an index out of range
__device__ __forceinline__ long long gq_mix_formula(const GqeDev &G, const long long *__restrict__ fo, long long B, int F,
                                                    long long r) {
    long long q = r;
    if (G.form == 0) {
        q = G.qrow[r];
        if (q < 0 || q >= B) return -1;
    }
    const long long f = fo[q];
    return f < 0 || f >= F ? -1 : f;
}

// this workgroup's stretch of P rows (mix_find_stretch): workgroup 16 k + j owns the j-th stretch of block k
__device__ __forceinline__ bool gq_mix_stretch(const GqeDev &G, const long long *__restrict__ fo, long long B, int F,
                                               long long &first, long long &end, int &fi) {
    return mix_find_stretch((long long)(blockIdx.x >> 4) * GQ_ROWS, GQ_ROWS, G.Rp, blockIdx.x & 15,
                            [&](long long r) { return gq_mix_formula(G, fo, B, F, r); }, first, end, fi);
}

// rows [0, cnt) of a tile -> rows [first, first + cnt) of a [Rp16, D] state: a stretch's own rows (the zero rows that pad
// its tile belong to a neighbouring stretch's state)
__device__ __forceinline__ void gq_store_rows(const float *tile, int LDX, float *g, long long first, int cnt, int D) {
    const int per = D / 4;
    for (int e = threadIdx.x; e < cnt * per; e += 256) {
        const int i = e / per, c = (e % per) * 4;
        *reinterpret_cast<f32x4 *>(g + (first + i) * D + c) = *reinterpret_cast<const f32x4 *>(tile + i * LDX + c);
    }
}

// The training states of the mixed calls (gqe_mixed_train.h) by arithmetic, not through GqeDev's offset arrays (the mixed
// kernels write their formula's tables into their copy of the record; an array of it indexed by a loop variable would then
// live in scratch): G.save holds the mask of the sites the query type uses, slot k is the k-th of them, X[k] sits at
// 2 k blk, dY[k] at (2 k + 1) blk and T[b] at (2 slots + b) blk, blk = Rp16 * D floats.
__device__ __forceinline__ long long gq_mix_x_off(const GqeDev &G, int site) {
    return 2ll * __builtin_popcount((unsigned)G.save & ((1u << site) - 1u)) * (G.Rp16 * G.D);
}
__device__ __forceinline__ long long gq_mix_dy_off(const GqeDev &G, int site) { return gq_mix_x_off(G, site) + G.Rp16 * G.D; }
__device__ __forceinline__ long long gq_mix_t_off(const GqeDev &G, int b) {
    return (2ll * __builtin_popcount((unsigned)G.save) + b) * (G.Rp16 * G.D);
}

// SAVE = 1 (mpqe_gqe_fwd_mixed_save): the states of mpqe_gqe_fwd(save_states = 1), by P row of the concatenation; the
// arithmetic, and so every score's bits, is that of SAVE = 0.
// KIND 0: SAVE = 0; 1: SAVE = 1; 2 (mpqe_gqe_embed_mixed, intersection form): SAVE = 0 and, as gqe_fwd_kernel's EMBED, the
// rows the forward would score go to `scores` as [Rp, D] -- a stretch writes its own rows, a bad formula's rows are zeros.
template <int DOT, int KIND>
__global__ __launch_bounds__(256) void gqe_fwd_mixed_kernel(GqeDev G, const GqeMixDesc *__restrict__ desc,
                                                            const long long *__restrict__ fo, long long B, int F,
                                                            float *__restrict__ scores) {
    constexpr int SAVE = KIND == 1 ? 1 : 0;
    constexpr int EMBED = KIND == 2 ? 1 : 0;
    __shared__ __attribute__((aligned(16))) float lds[3 * GQ_ROWS * GQ_LDXMAX];
    const int D = G.D, LDX = D + 4, per = D / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long first, end;
    int fi;
    if (!gq_mix_stretch(G, fo, B, F, first, end, fi)) return;
    fi = __builtin_amdgcn_readfirstlane(fi);
    if (fi < 0) {
        if (threadIdx.x == 0) flag_error(G.err, MPQE_FLAG_BAD_INDEX);
        if (EMBED) {
            for (long long e = threadIdx.x; e < (end - first) * D; e += 256) scores[first * D + e] = 0.f;
            return;
        }
        for (int i = wave; i < GQ_ROWS; i += 4) {
            const long long q = first + i;
            if (q >= end) continue;
            if (lane == 0) scores[q] = 0.f;
            if (G.form == 0) continue;
            long long lo, hi;
            gq_neg_range(G, q, lane, lo, hi);
            for (long long r = lo + lane; r < hi; r += 64) scores[r] = 0.f;
        }
        return;
    }
    const GqeMixDesc &M = desc[fi];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        G.tab[t] = M.tab[t];
        G.tab_rows[t] = M.tab_rows[t];
    }
    float *cur = lds, *nxt = lds + GQ_ROWS * LDX, *agg = lds + 2 * GQ_ROWS * LDX;
    const int nrow = (int)(end - first);      // (SAVE: the stretch's own rows)

#pragma unroll
    for (int b = 0; b < 3; ++b) {
        if (b >= G.nb) break;
        gq_gather(G, cur, LDX, G.p_ids + (long long)b * G.Rp, b, first, end);
        __syncthreads();
        for (int s = 0; s < G.bn[b]; ++s) {
            const int site = 3 * b + s;
            if (G.op) {
                if (SAVE && G.op == 2) {
                    gq_store_rows(cur, LDX, G.ws + gq_mix_x_off(G, site), first, nrow, D);
                    __syncthreads();
                }
                gq_vec(cur, LDX, M.w[site], D, G.op, nullptr, first);
                __syncthreads();
                continue;
            }
            if (SAVE) gq_store_rows(cur, LDX, G.ws + gq_mix_x_off(G, site), first, nrow, D);
            gq_mm(cur, nxt, M.w[site], D, LDX, M.T[site], 0);
            __syncthreads();
            float *t = cur; cur = nxt; nxt = t;
        }
        if (G.nb < 2) break;
        if (G.has_pre) {
            if (SAVE) gq_store_rows(cur, LDX, G.ws + gq_mix_x_off(G, GQ_SITE_PRE + b), first, nrow, D);
            gq_mm(cur, nxt, M.w[GQ_SITE_PRE + b], D, LDX, 1, 1);
            __syncthreads();
            float *t = cur; cur = nxt; nxt = t;
        }
        if (SAVE) gq_store_rows(cur, LDX, G.ws + gq_mix_t_off(G, b), first, nrow, D);
        for (int e = threadIdx.x; e < GQ_ROWS * per; e += 256) {
            const int o = (e / per) * LDX + (e % per) * 4;
            f32x4 v = *reinterpret_cast<const f32x4 *>(cur + o);
            if (b > 0) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(agg + o);
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = G.agg ? (v[u] < a[u] ? v[u] : a[u]) : a[u] + v[u];
            }
            if (!G.agg && b == G.nb - 1) {
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] /= (float)G.nb;
            }
            *reinterpret_cast<f32x4 *>(agg + o) = v;
        }
        __syncthreads();
    }
    if (G.nb >= 2) {
        float *t = cur; cur = agg; agg = t;
        if (G.has_post) {
            if (SAVE) gq_store_rows(cur, LDX, G.ws + gq_mix_x_off(G, GQ_SITE_POST), first, nrow, D);
            gq_mm(cur, nxt, M.w[GQ_SITE_POST], D, LDX, 1, 0);
            __syncthreads();
            t = cur; cur = nxt; nxt = t;
        }
    }
    for (int s = 0; s < G.ntail; ++s) {
        const int site = GQ_SITE_TAIL + s;
        if (G.op) {
            if (SAVE && G.op == 2) {
                gq_store_rows(cur, LDX, G.ws + gq_mix_x_off(G, site), first, nrow, D);
                __syncthreads();
            }
            gq_vec(cur, LDX, M.w[site], D, G.op, nullptr, first);
            __syncthreads();
            continue;
        }
        if (SAVE) gq_store_rows(cur, LDX, G.ws + gq_mix_x_off(G, site), first, nrow, D);
        gq_mm(cur, nxt, M.w[site], D, LDX, M.T[site], 0);
        __syncthreads();
        float *t = cur; cur = nxt; nxt = t;
    }
    if (SAVE) gq_store_rows(cur, LDX, G.ws + G.pfin_off, first, nrow, D);
    if (EMBED) {
        gq_store_rows(cur, LDX, scores, first, nrow, D);
        return;
    }

    for (int i = wave; i < GQ_ROWS; i += 4) {
        const long long q = first + i;
        if (q >= end) continue;
        f32x4 p = {0.f, 0.f, 0.f, 0.f};
        if (lane * 4 < D) p = *reinterpret_cast<const f32x4 *>(cur + i * LDX + lane * 4);
        if (G.form == 0) {
            const float s = gq_score<DOT>(G, p, gq_e_row(G, q, lane), nullptr, nullptr, nullptr);
            if (lane == 0) scores[q] = s;
        } else {
            long long lo, hi;
            gq_neg_range(G, q, lane, lo, hi);
            for (long long r = q;;) {
                const float s = gq_score<DOT>(G, p, gq_e_row(G, r, lane), nullptr, nullptr, nullptr);
                if (lane == 0) scores[r] = s;
                r = r == q ? lo : r + 1;
                if (r >= hi) break;
            }
        }
    }
}

static inline size_t gqe_mixed_desc_size(int64_t F) { return align_up((size_t)F * sizeof(GqeMixDesc), 256); }

extern "C" size_t mpqe_gqe_mixed_desc_bytes(int64_t num_formulas) {
    if (num_formulas < 1 || num_formulas >= ((int64_t)1 << 24)) return 0;
    return gqe_mixed_desc_size(num_formulas);
}

// the ints of a programme that the query type fixes: everything but the tables, the codes and the pre / post indices
static bool gqe_mixed_same_shape(const int32_t *a, const int32_t *b) {
    if (a[0] != b[0] || a[1] != b[1] || a[2] != b[2] || a[5] != b[5] || a[7] != b[7]) return false;
    if ((a[27] == 1) != (b[27] == 1) || (a[3] >= 0) != (b[3] >= 0) || (a[4] >= 0) != (b[4] >= 0)) return false;
    for (int k = 0; k < a[1] && k < 3; ++k)
        if (a[9 + 5 * k] != b[9 + 5 * k]) return false;
    return true;
}

extern "C" int mpqe_gqe_mixed_desc_build(const int32_t *progs_host, int64_t num_formulas, const float *const *tables_host,
                                         const int64_t *table_rows_host, int num_tables, const float *const *mats_host,
                                         int num_mats, int64_t dim, void *desc, size_t desc_bytes, void *stream) {
    if (!progs_host || num_tables < 1 || num_mats < 0 || !desc) return MPQE_ERR_INVALID_ARG;
    if (num_formulas < 1 || num_formulas >= ((int64_t)1 << 24)) return MPQE_ERR_INVALID_ARG;
    if ((uintptr_t)desc % 256 != 0) return MPQE_ERR_INVALID_ARG;
    GqeMixDesc *image = new (std::nothrow) GqeMixDesc[(size_t)num_formulas];
    if (!image) return MPQE_ERR_INVALID_ARG;
    memset(image, 0, (size_t)num_formulas * sizeof(GqeMixDesc));
    int st = MPQE_OK;
    for (int64_t f = 0; f < num_formulas && st == MPQE_OK; ++f) {
        const int32_t *prog = progs_host + f * MPQE_GQE_PROG_INTS;
        GqeHost H;
        // (the sizes of a call are not known here: one row stands for them; the form decides which of them must agree)
        st = gqe_plan(prog, num_tables, num_mats, dim, 1, 1, 1, &H);
        if (st != MPQE_OK) break;
        if (!gqe_mixed_same_shape(progs_host, prog)) {
            st = MPQE_ERR_INVALID_ARG;
            break;
        }
        st = gqe_bind(&H, tables_host, table_rows_host, nullptr, 0, mats_host, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr,
                      nullptr, true);
        if (st != MPQE_OK) break;
        // (p_only leaves the E side's table out)
        H.G.tab[3] = tables_host[H.G.tmode[3]];
        H.G.tab_rows[3] = table_rows_host[H.G.tmode[3]];
        if (!H.G.tab[3] || H.G.tab_rows[3] < 0 || (uintptr_t)H.G.tab[3] % 16 != 0) {
            st = MPQE_ERR_INVALID_ARG;
            break;
        }
        GqeMixDesc &M = image[f];
        for (int t = 0; t < 4; ++t) {
            M.tab[t] = H.G.tab[t];
            M.tab_rows[t] = H.G.tab_rows[t];
        }
        for (int s = 0; s < GQ_SITES; ++s) {
            M.w[s] = H.G.w[s];
            M.T[s] = H.site_mat[s] < 0 ? 0 : H.site_T[s];
        }
    }
    if (st == MPQE_OK && desc_bytes < gqe_mixed_desc_size(num_formulas)) st = MPQE_ERR_WORKSPACE;
    if (st == MPQE_OK &&
        hipMemcpyAsync(desc, image, (size_t)num_formulas * sizeof(GqeMixDesc), hipMemcpyHostToDevice, as_stream(stream)) !=
            hipSuccess)
        st = MPQE_ERR_LAUNCH;
    // (the copy reads pageable memory: it has left `image` when the call returns)
    delete[] image;
    return st;
}

// the mixed entry points: mpqe_gqe_fwd_mixed, and training on such windows (index block, forward with states, backward)
#include "gqe_mixed_train.h"

extern "C" int mpqe_gqe_bwd(const int32_t *prog_host, const float *const *tables_host, const int64_t *table_rows_host,
                            int num_tables, const int64_t *node_map, int64_t node_map_len, const float *const *mats_host,
                            int num_mats, int64_t dim, const int64_t *p_ids, int64_t p_rows, const int64_t *e_ids,
                            int64_t e_rows, const int64_t *qrow, const int64_t *neg_off, int64_t n, float eps,
                            const float *grad_scores, float *const *grad_tables_host, float *const *grad_mats_host,
                            void *workspace, size_t workspace_bytes, int32_t *err, void *stream) {
    if (num_tables < 1 || num_mats < 0 || !grad_scores || !grad_tables_host || !grad_mats_host) return MPQE_ERR_INVALID_ARG;
    GqeHost H;
    int st = gqe_plan(prog_host, num_tables, num_mats, dim, p_rows, e_rows, n, &H);
    if (st != MPQE_OK) return st;
    st = gqe_bind(&H, tables_host, table_rows_host, node_map, node_map_len, mats_host, p_ids, e_ids, qrow, neg_off, eps,
                  workspace, err);
    if (st != MPQE_OK) return st;
    if (!workspace || (uintptr_t)workspace % 256 != 0) return MPQE_ERR_INVALID_ARG;
    if (workspace_bytes < H.total) return MPQE_ERR_WORKSPACE;
    GqeDev &G = H.G;
    bool any_table = false;
    for (int t = 0; t < 4; ++t) {
        if (t < 3 && t >= G.nb) continue;
        G.gtab[t] = grad_tables_host[G.tmode[t]];
        if (G.gtab[t] && (uintptr_t)G.gtab[t] % 16 != 0) return MPQE_ERR_INVALID_ARG;
        any_table = any_table || G.gtab[t];
    }
    for (int s = 0; s < GQ_SITES; ++s) {
        float *g = H.site_mat[s] < 0 ? nullptr : grad_mats_host[H.site_mat[s]];
        if (g && (uintptr_t)g % 16 != 0) return MPQE_ERR_INVALID_ARG;
    }
    hipStream_t s = as_stream(stream);
    if (G.dot)
        hipLaunchKernelGGL(gqe_bwd_kernel<1>, dim3((unsigned)(G.Rp16 / GQ_ROWS)), dim3(256), 0, s, G, grad_scores);
    else
        hipLaunchKernelGGL(gqe_bwd_kernel<0>, dim3((unsigned)(G.Rp16 / GQ_ROWS)), dim3(256), 0, s, G, grad_scores);
    if (any_table) {
        const long long n_ent = (long long)G.nb * G.Rp + G.n;
        hipLaunchKernelGGL(gqe_keys_kernel, dim3((unsigned)((n_ent + 255) / 256)), dim3(256), 0, s, G, n_ent);
        hipLaunchKernelGGL(gqe_rows_kernel, dim3((unsigned)((n_ent + 3) / 4)), dim3(256), 0, s, G, n_ent);
    }
    st = mpqe_launch_status();
    if (st != MPQE_OK) return st;
    // matrix gradients, site after site (stream order = programme order): Y = X . M^T: gM = dY^T . X; Y = X . M: gM = X^T . dY
    char *lin = reinterpret_cast<char *>(workspace) + H.lin_off;
    if (G.op) {
        // vector gradients: one launch, the sites in programme order inside it
        GqeVecFin F;
        F.n = 0;
        for (int site = 0; site < GQ_SITES; ++site) {
            if (H.site_mat[site] < 0 || !gqe_vec_site(G.op, site)) continue;
            float *gv = grad_mats_host[H.site_mat[site]];
            if (!gv) continue;
            F.part[F.n] = G.ws + G.part_off[site];
            F.grad[F.n] = gv;
            ++F.n;
        }
        if (F.n > 0) {
            hipLaunchKernelGGL(gqe_vec_final_kernel, dim3(1), dim3(4 * GQ_MAXD), 0, s, F, (long long)(G.Rp16 / GQ_ROWS), G.D);
            st = mpqe_launch_status();
            if (st != MPQE_OK) return st;
        }
    }
    for (int site = 0; site < GQ_SITES; ++site) {
        if (H.site_mat[site] < 0 || gqe_vec_site(G.op, site)) continue;
        float *gm = grad_mats_host[H.site_mat[site]];
        if (!gm) continue;
        const float *X = G.ws + G.x_off[site], *dY = G.ws + G.dy_off[site];
        const bool T = H.site_T[site] != 0;
        st = mpqe_linear_bwd(T ? X : dY, p_rows, G.w[site], dim, nullptr, T ? dY : X, dim, dim, 0, 0, nullptr, gm, dim, nullptr,
                             lin, H.lin_bytes, stream);
        if (st != MPQE_OK) return st;
    }
    return MPQE_OK;
}

// ------------------------------------------------------------------------------------------------ branch aggregate alone
// out = mean / min of two or three equally shaped arrays, element by element (decoders.py:293-298, 313-318: torch.stack +
// agg_func(dim=0)); the backward gives a minimum's gradient to the first branch that holds it. The composed path's op.
__global__ __launch_bounds__(256) void branch_agg_fwd_kernel(const float *__restrict__ x0, const float *__restrict__ x1,
                                                             const float *__restrict__ x2, long long count, int agg,
                                                             float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float a = x0[i], b = x1[i];
    float v;
    if (agg) {
        v = b < a ? b : a;
        if (x2) v = x2[i] < v ? x2[i] : v;
    } else {
        v = x2 ? (a + b + x2[i]) / 3.f : (a + b) / 2.f;
    }
    out[i] = v;
}
__global__ __launch_bounds__(256) void branch_agg_bwd_kernel(const float *__restrict__ x0, const float *__restrict__ x1,
                                                             const float *__restrict__ x2, long long count, int agg,
                                                             const float *__restrict__ g, float *__restrict__ g0,
                                                             float *__restrict__ g1, float *__restrict__ g2) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float gi = g[i];
    float r0, r1, r2;
    if (agg) {
        int win = 0;
        float m = x0[i];
        if (x1[i] < m) {
            m = x1[i];
            win = 1;
        }
        if (x2 && x2[i] < m) win = 2;
        r0 = win == 0 ? gi : 0.f;
        r1 = win == 1 ? gi : 0.f;
        r2 = win == 2 ? gi : 0.f;
    } else {
        r0 = r1 = r2 = gi / (x2 ? 3.f : 2.f);
    }
    if (g0) g0[i] = r0;
    if (g1) g1[i] = r1;
    if (g2 && x2) g2[i] = r2;
}

extern "C" int mpqe_branch_agg_fwd(const float *x0, const float *x1, const float *x2, int64_t count, int agg, float *out,
                                   void *stream) {
    if (count < 0 || agg < 0 || agg > 1) return MPQE_ERR_INVALID_ARG;
    if (count == 0) return MPQE_OK;
    if (!x0 || !x1 || !out) return MPQE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(branch_agg_fwd_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, as_stream(stream), x0, x1,
                       x2, (long long)count, agg, out);
    return mpqe_launch_status();
}

extern "C" int mpqe_branch_agg_bwd(const float *x0, const float *x1, const float *x2, int64_t count, int agg,
                                   const float *grad_out, float *grad_x0, float *grad_x1, float *grad_x2, void *stream) {
    if (count < 0 || agg < 0 || agg > 1) return MPQE_ERR_INVALID_ARG;
    if (count == 0) return MPQE_OK;
    if (!x0 || !x1 || !grad_out) return MPQE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(branch_agg_bwd_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, as_stream(stream), x0, x1,
                       x2, (long long)count, agg, grad_out, grad_x0, grad_x1, grad_x2);
    return mpqe_launch_status();
}
