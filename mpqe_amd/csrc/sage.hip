// The neighbourhood-aggregating entity encoder of the reference (utils.get_encoder utils.py:97-130, Encoder
// encoders.py:47-129, MeanAggregator aggregators.py:17-68) on the device KG index. Conventions of kg.hip / gqe.hip: table
// ROWS everywhere, host arrays of device pointers, arguments checked before any launch, a bad offset / row flagged
// (MPQE_FLAG_BAD_INDEX) and not followed, every word of every output written, no float atomics.
//
// mpqe_kg_sample_neighbours  one lane per (relation, batch position): the count rule of aggregators.py:51-53 in double,
//   then either the whole list or the first k images of the samplers' keyed bijection (kg_stream.h) over the list's
//   positions. Integer work, latency bound, nothing shared between lanes.
//
// mpqe_sage_fwd  one launch. As in gqe.hip a workgroup owns 16 batch rows. The compress matrix's column blocks are walked
//   in order; per block the 16 mean rows are formed in LDS (every thread owns 4 columns of one row and adds its sampled
//   rows in slot order, four 16-byte loads in flight), then multiplied into the accumulators on v_mfma_f32_16x16x4_f32
//   (gq_mm's lane map: wave w owns the column blocks w, w + 4, ..; W is read in place, 16 bytes along k). The
//   concatenation exists only as that sequence of LDS tiles. The z tile goes through LDS once more so that one wave sees a
//   whole row for the normalisation (the arithmetic of layernorm_relu_fwd_kernel, so its backward kernel serves).
//
// mpqe_sage_bwd  the ReLU / LayerNorm backward and the two products are the library's (mpqe_layernorm_relu_bwd,
//   mpqe_linear_bwd over the saved feature rows: grad_W on its fixed-order tiles, g_feat = grad_z . W). Row gradients: one
//   (table, row) key per entry (sage_keys_kernel), a stable radix sort (radix_sort.h), then one wave per run of equal keys
//   adds the run's entries in entry order and is the row's only writer (sage_rows_kernel). An entry's gradient is read from
//   g_feat where it lies and scaled on the fly; no per-entry row is stored.
#include <math.h>
#include <string.h>

#include "gemm_core.h"
#include "kg_stream.h"
#include "radix_sort.h"

#define SG_ROWS 16
#define SG_MAXD 256
#define SG_LDXMAX (SG_MAXD + 4)
#define SG_MAX_RELS MPQE_SAGE_MAX_RELS
#define SG_MAX_BLOCKS (SG_MAX_RELS + 1)
#define SG_MAX_KEEP MPQE_SAGE_MAX_KEEP
#define SG_MAX_BATCH ((int64_t)1 << 30)

// ------------------------------------------------------------------------------------------------ the sampler
struct SnRel {
    const long long *off;       // [rows(src) + 1]
    const long long *rows;      // [edges], rows of the destination mode
    long long edges, n_dst;
    unsigned long long index;   // the relation's index in the KG index: the high half of the stream's slot
};
struct SnDev {
    SnRel rel[SG_MAX_RELS];
    long long n_src, B;
    int R, max_keep;
    double keep_prob;
    unsigned long long seed;
};

__global__ __launch_bounds__(256) void kg_sample_neighbours_kernel(SnDev S, const long long *__restrict__ rows,
                                                                   long long *__restrict__ neigh, int *__restrict__ counts,
                                                                   int32_t *err) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)blockIdx.y;
    if (b >= S.B) return;
    const SnRel &r = S.rel[i];
    long long *slots = neigh + ((long long)i * S.B + b) * S.max_keep;
    const long long x = rows[b];
    long long lo = 0, len = 0;
    if (x >= S.n_src) {
        flag_error(err, MPQE_FLAG_BAD_INDEX);
    } else if (x >= 0) {
        lo = r.off[x];
        const long long hi = r.off[x + 1];
        if (lo < 0 || hi < lo || hi > r.edges) flag_error(err, MPQE_FLAG_BAD_INDEX);
        else len = hi - lo;
    }
    int k = 0;
    if (len > 0) {
        // min(int(math.ceil(len(nb) * keep_prob)), max_keep), aggregators.py:51-53: one double product, its ceiling
        const double want = ceil((double)len * S.keep_prob);
        k = want < (double)S.max_keep ? (int)want : S.max_keep;
        int h = 1;
        while (((long long)1 << (2 * h)) < len) ++h;
        const unsigned long long key = mpqe_mix64(S.seed ^ mpqe_mix64((r.index << 32) | (unsigned long long)b));
        for (int j = 0; j < k; ++j) {
            const long long at = k < len ? kgs_permute(key, len, h, j) : j;
            long long y = r.rows[lo + at];
            if (y < 0 || y >= r.n_dst) {
                flag_error(err, MPQE_FLAG_BAD_INDEX);
                y = -1;
            }
            slots[j] = y;
        }
    }
    for (int j = k; j < S.max_keep; ++j) slots[j] = -1;
    counts[(long long)i * S.B + b] = k;
}

extern "C" int mpqe_kg_sample_neighbours(const int64_t *const *rel_offsets_host, const int64_t *const *rel_rows_host,
                                         const int64_t *rel_edges_host, const int32_t *rel_src_mode_host,
                                         const int32_t *rel_dst_mode_host, int num_rels, const int64_t *mode_rows_host,
                                         int num_modes, const int32_t *use_rels_host, int R, const int64_t *rows, int64_t B,
                                         double keep_prob, int max_keep, uint64_t seed, int64_t *neigh, int32_t *counts,
                                         int32_t *err, void *stream) {
    if (num_rels < 1 || num_modes < 1 || num_modes > 16 || R < 1 || R > SG_MAX_RELS) return MPQE_ERR_INVALID_ARG;
    if (!rel_offsets_host || !rel_rows_host || !rel_edges_host || !rel_src_mode_host || !rel_dst_mode_host ||
        !mode_rows_host || !use_rels_host)
        return MPQE_ERR_INVALID_ARG;
    if (max_keep < 1 || max_keep > SG_MAX_KEEP || !(keep_prob > 0.0 && keep_prob <= 1.0)) return MPQE_ERR_INVALID_ARG;
    if (B < 0 || B > SG_MAX_BATCH) return MPQE_ERR_INVALID_ARG;
    for (int m = 0; m < num_modes; ++m)
        if (mode_rows_host[m] < 1 || mode_rows_host[m] > ((int64_t)1 << 30)) return MPQE_ERR_INVALID_ARG;
    SnDev S;
    memset(&S, 0, sizeof(S));
    int src_mode = -1;
    for (int i = 0; i < R; ++i) {
        const int ri = use_rels_host[i];
        if (ri < 0 || ri >= num_rels) return MPQE_ERR_INVALID_ARG;
        const int src = rel_src_mode_host[ri], dst = rel_dst_mode_host[ri];
        if (src < 0 || src >= num_modes || dst < 0 || dst >= num_modes || (i > 0 && src != src_mode)) return MPQE_ERR_INVALID_ARG;
        src_mode = src;
        if (!rel_offsets_host[ri] || rel_edges_host[ri] < 0 || (rel_edges_host[ri] > 0 && !rel_rows_host[ri]))
            return MPQE_ERR_INVALID_ARG;
        S.rel[i].off = reinterpret_cast<const long long *>(rel_offsets_host[ri]);
        S.rel[i].rows = reinterpret_cast<const long long *>(rel_rows_host[ri]);
        S.rel[i].edges = rel_edges_host[ri];
        S.rel[i].n_dst = mode_rows_host[dst];
        S.rel[i].index = (unsigned long long)ri;
    }
    if (B == 0) return MPQE_OK;
    if (!rows || !neigh || !counts) return MPQE_ERR_INVALID_ARG;
    S.n_src = mode_rows_host[src_mode];
    S.B = B;
    S.R = R;
    S.max_keep = max_keep;
    S.keep_prob = keep_prob;
    S.seed = seed;
    hipLaunchKernelGGL(kg_sample_neighbours_kernel, dim3((unsigned)((B + 255) / 256), (unsigned)R), dim3(256), 0,
                       as_stream(stream), S, reinterpret_cast<const long long *>(rows), reinterpret_cast<long long *>(neigh),
                       reinterpret_cast<int *>(counts), err);
    return mpqe_launch_status();
}

// ------------------------------------------------------------------------------------------------ the encoder
struct SageDev {
    const float *src[SG_MAX_BLOCKS];        // block r's source matrix [src_rows, din]
    float *gsrc[SG_MAX_BLOCKS];             // its gradient (backward; NULL = not wanted)
    long long src_rows[SG_MAX_BLOCKS], pad[SG_MAX_BLOCKS];
    int tab[SG_MAX_BLOCKS];                 // its index in tables_host: the high part of a row's key
    int R, din, dout, max_keep, ln, save, num_tables, row_bits;
    long long B, K;                         // K = (R + 1) din
    const long long *neigh, *self_rows;
    const int *counts;
    const float *W, *gamma, *beta;
    float eps;
    float *feat, *z, *stats;                // workspace: [B, K], [B, dout], [B, 2]
    int32_t *err;
};

// counts[r, b] as the kernels take it: outside [0, max_keep] it is flagged (by the forward) and taken as 0
__device__ __forceinline__ int sg_count(const SageDev &S, int blk, long long b, int32_t *err) {
    const int c = S.counts[(long long)blk * S.B + b];
    if (c < 0 || c > S.max_keep) {
        flag_error(err, MPQE_FLAG_BAD_INDEX);
        return 0;
    }
    return c;
}

__global__ __launch_bounds__(256) void sage_fwd_kernel(SageDev S, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[SG_ROWS * SG_LDXMAX];      // the block's feature rows [16][din + 4]
    __shared__ __attribute__((aligned(16))) float zt[SG_ROWS * SG_LDXMAX];        // z [16][dout + 4]
    const int din = S.din, dout = S.dout, LDA = din + 4, LDZ = dout + 4, per = din / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, kq = lane >> 4;
    const long long i0 = (long long)blockIdx.x * SG_ROWS;
    f32x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int blk = 0; blk <= S.R; ++blk) {
        const float *src = S.src[blk];
        const long long src_rows = S.src_rows[blk];
        for (int e = threadIdx.x; e < SG_ROWS * per; e += 256) {
            const int i = e / per, c = (e % per) * 4;
            const long long b = i0 + i;
            int32_t *err = c == 0 ? S.err : nullptr;        // (one lane of a row speaks for it)
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (b < S.B) {
                if (blk < S.R) {
                    const int cnt = sg_count(S, blk, b, err);
                    if (cnt == 0) {
                        v = gload4(src + S.pad[blk] * din + c);
                    } else {
                        const long long *nb = S.neigh + ((long long)blk * S.B + b) * S.max_keep;
                        for (int s0 = 0; s0 < cnt; s0 += 4) {
                            f32x4 q[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                q[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                                if (s0 + u < cnt) {
                                    const long long row = nb[s0 + u];
                                    if (row >= 0 && row < src_rows) q[u] = gload4(src + row * din + c);
                                    else flag_error(err, MPQE_FLAG_BAD_INDEX);
                                }
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                v[0] += q[u][0]; v[1] += q[u][1]; v[2] += q[u][2]; v[3] += q[u][3];
                            }
                        }
                        const float inv = 1.f / (float)cnt;
                        v[0] *= inv; v[1] *= inv; v[2] *= inv; v[3] *= inv;
                    }
                } else {
                    long long row = S.self_rows[b];
                    if (row < 0) row = S.pad[blk];
                    if (row < src_rows) v = gload4(src + row * din + c);
                    else flag_error(err, MPQE_FLAG_BAD_INDEX);
                }
                if (S.save) *reinterpret_cast<f32x4 *>(S.feat + b * S.K + (long long)blk * din + c) = v;
            }
            *reinterpret_cast<f32x4 *>(tile + i * LDA + c) = v;
        }
        __syncthreads();
        const float *Wb = S.W + (long long)blk * din;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int cb = wave + 4 * q;
            if (cb < dout / 16) {
                const float *wrow = Wb + (long long)(cb * 16 + j) * S.K;
                for (int t = 0; t < din / 16; ++t) {
                    const int k0 = 16 * t + 4 * kq;
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(tile + j * LDA + k0);
                    const f32x4 w = gload4(wrow + k0);
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], w[u], acc[q], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int cb = wave + 4 * q;
        if (cb < dout / 16) {
#pragma unroll
            for (int r = 0; r < 4; ++r) zt[(4 * kq + r) * LDZ + cb * 16 + j] = acc[q][r];
        }
    }
    __syncthreads();
    // one wave per row: ReLU, or the normalisation of layernorm_relu_fwd_kernel and the ReLU
    for (int i = wave; i < SG_ROWS; i += 4) {
        const long long b = i0 + i;
        if (b >= S.B) continue;
        const float *zr = zt + i * LDZ;
        float mean = 0.f, inv = 1.f;
        if (S.ln) {
            float s = 0.f;
            for (int c = lane; c < dout; c += 64) s += zr[c];
            mean = wave_sum(s) / (float)dout;
            float q = 0.f;
            for (int c = lane; c < dout; c += 64) {
                const float d = zr[c] - mean;
                q += d * d;
            }
            const float sd = sqrtf(wave_sum(q) / (float)(dout - 1));
            inv = 1.f / (sd + S.eps);
        }
        for (int c = lane; c < dout; c += 64) {
            float v = zr[c];
            if (S.save) S.z[b * dout + c] = v;
            if (S.ln) v = S.gamma[c] * ((v - mean) * inv) + S.beta[c];
            out[b * dout + c] = v > 0.f ? v : 0.f;
        }
        if (S.save && S.ln && lane == 0) {
            S.stats[2 * b] = mean;
            S.stats[2 * b + 1] = inv;
        }
    }
}

// entry e of the row gradients -> its block, batch position and scale; the row it belongs to, or -1 (an unused slot, a row
// the forward flagged). Entries: (r, b, s) for r < R in that order, then the self rows.
__device__ __forceinline__ long long sg_entry(const SageDev &S, long long e, int &blk, long long &b, float &scale) {
    const long long per_rel = S.B * S.max_keep, n_rel = (long long)S.R * per_rel;
    scale = 1.f;
    long long row;
    if (e < n_rel) {
        blk = (int)(e / per_rel);
        const long long rem = e % per_rel;
        b = rem / S.max_keep;
        const int s = (int)(rem % S.max_keep);
        const int cnt = sg_count(S, blk, b, nullptr);
        if (cnt == 0) {
            if (s != 0) return -1;
            row = S.pad[blk];
        } else {
            if (s >= cnt) return -1;
            row = S.neigh[e];
            scale = 1.f / (float)cnt;
        }
    } else {
        blk = S.R;
        b = e - n_rel;
        row = S.self_rows[b];
        if (row < 0) row = S.pad[blk];
    }
    return row >= 0 && row < S.src_rows[blk] ? row : -1;
}

// key = table << row_bits | row; entries without a row (or of a table whose gradient is not wanted) carry the table index
// num_tables and sort behind every real key
__global__ __launch_bounds__(256) void sage_keys_kernel(SageDev S, long long n_ent, long long *__restrict__ keys) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ent) return;
    int blk;
    long long b;
    float scale;
    const long long row = sg_entry(S, e, blk, b, scale);
    long long key = (long long)S.num_tables << S.row_bits;
    if (row >= 0 && S.gsrc[blk]) key = ((long long)S.tab[blk] << S.row_bits) | row;
    keys[e] = key;
}

// one wave per sorted position: the first position of a run of equal keys adds the run's entries in sorted (= entry) order
// and adds the sum to the row of the table's gradient -- the row's only writer. The run is taken 64 entries at a time: every
// lane decodes one entry (position -> block, batch row, scale: three dependent loads), then the wave walks the 64 records
// by broadcast, so that the loads of g_feat -- one per entry -- do not wait on one another. (A table's padding row can own
// a run of thousands of entries at depth >= 2, where every unused slot is a null node.)
__global__ __launch_bounds__(256) void sage_rows_kernel(SageDev S, long long n_ent, const long long *__restrict__ keys,
                                                        const int *__restrict__ perm, const float *__restrict__ gfeat) {
    const long long k = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, c = lane * 4;
    if (k >= n_ent) return;
    const long long key = keys[k];
    if ((key >> S.row_bits) >= S.num_tables) return;
    if (k > 0 && keys[k - 1] == key) return;
    const long long row = key & ((1ll << S.row_bits) - 1ll);
    const bool cols = c < S.din;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int blk0 = 0;
    for (long long p0 = k;; p0 += 64) {
        const long long p = p0 + lane;
        const bool mine = p < n_ent && keys[p] == key;          // (a run is contiguous: the lanes that hold it are a prefix)
        int blk_l = 0, b_l = 0;
        float scale_l = 0.f;
        if (mine) {
            long long b;
            (void)sg_entry(S, (long long)perm[p], blk_l, b, scale_l);
            b_l = (int)b;
        }
        const int n = (int)wave_sum(mine ? 1.f : 0.f);
        if (p0 == k) blk0 = __shfl(blk_l, 0, 64);
        for (int l = 0; l < n; ++l) {
            const int blk = __shfl(blk_l, l, 64), b = __shfl(b_l, l, 64);
            const float scale = __shfl(scale_l, l, 64);
            if (cols) {
                const f32x4 g = gload4(gfeat + (long long)b * S.K + (long long)blk * S.din + c);
                acc[0] += g[0] * scale; acc[1] += g[1] * scale; acc[2] += g[2] * scale; acc[3] += g[3] * scale;
            }
        }
        if (n < 64) break;
    }
    if (!cols) return;
    float *o = S.gsrc[blk0] + row * S.din + c;      // (every block of one table names the same gradient)
    f32x4 old = *reinterpret_cast<const f32x4 *>(o);
    old[0] += acc[0]; old[1] += acc[1]; old[2] += acc[2]; old[3] += acc[3];
    *reinterpret_cast<f32x4 *>(o) = old;
}

// ------------------------------------------------------------------------------------------------ host side
struct SageLayout {
    size_t feat, z, stats, dz, gfeat, dummy, keys_in, keys_out, perm, sort_tmp, ln_ws, lin_ws, total;
    size_t ln_bytes, lin_bytes;
    long long n_ent;
};

static int sage_layout(int64_t B, int R, int64_t din, int64_t dout, int max_keep, SageLayout *L) {
    if (B < 0 || B > SG_MAX_BATCH || R < 0 || R > SG_MAX_RELS || din <= 0 || dout <= 0 || max_keep < 1 || max_keep > SG_MAX_KEEP)
        return MPQE_ERR_INVALID_ARG;
    if (din % 16 != 0 || dout % 16 != 0 || din > SG_MAXD || dout > SG_MAXD) return MPQE_ERR_UNSUPPORTED;
    const long long n_ent = (long long)R * B * max_keep + B;
    if (n_ent >= (1ll << 31)) return MPQE_ERR_UNSUPPORTED;
    const size_t rows = (size_t)(B > 0 ? B : 1), K = (size_t)(R + 1) * (size_t)din, ne = (size_t)(n_ent > 0 ? n_ent : 1);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += align_up(bytes, 256);
        return at;
    };
    memset(L, 0, sizeof(*L));
    L->n_ent = n_ent;
    L->feat = take(rows * K * 4);
    L->z = take(rows * (size_t)dout * 4);
    L->stats = take(rows * 2 * 4);
    L->dz = take(rows * (size_t)dout * 4);
    L->gfeat = take(rows * K * 4);
    L->dummy = take(2 * (size_t)dout * 4);
    L->keys_in = take(ne * 8);
    L->keys_out = take(ne * 8);
    L->perm = take(ne * 4);
    L->sort_tmp = take(radix_sort_tmp_bytes<long long>((long long)ne));
    L->ln_bytes = mpqe_layernorm_relu_bwd_workspace_bytes((int64_t)rows, dout);
    L->ln_ws = take(L->ln_bytes);
    L->lin_bytes = mpqe_linear_bwd_workspace_bytes((int64_t)rows, (int64_t)K, dout);
    L->lin_ws = take(L->lin_bytes);
    L->total = off;
    return MPQE_OK;
}

extern "C" size_t mpqe_sage_workspace_bytes(int64_t batch, int num_rels, int64_t dim_in, int64_t dim_out, int max_keep) {
    SageLayout L;
    if (sage_layout(batch, num_rels, dim_in, dim_out, max_keep, &L) != MPQE_OK) return 0;
    return L.total;
}

static int bits_for(unsigned long long v) {      // the bits that hold every value 0 .. v
    int b = 1;
    while (b < 63 && (v >> b) != 0) ++b;
    return b;
}

// arguments -> device record and layout (no launch); with_ws: the workspace is needed and bound
static int sage_bind(const float *const *tables, const int64_t *table_rows, int num_tables, const int32_t *block_table,
                     const int64_t *block_pad, int R, const int64_t *neigh, const int32_t *counts, int max_keep,
                     const int64_t *self_rows, int64_t B, const float *W, int64_t din, int64_t dout, const float *gamma,
                     const float *beta, float eps, void *workspace, size_t workspace_bytes, bool with_ws, int32_t *err,
                     SageDev *S, SageLayout *L) {
    const int st = sage_layout(B, R, din, dout, max_keep, L);
    if (st != MPQE_OK) return st;
    if (!tables || !table_rows || num_tables < 1 || num_tables > SG_MAX_BLOCKS || !block_table || !block_pad || !W)
        return MPQE_ERR_INVALID_ARG;
    if ((gamma == nullptr) != (beta == nullptr) || (uintptr_t)W % 16 != 0) return MPQE_ERR_INVALID_ARG;
    memset(S, 0, sizeof(*S));
    long long max_rows = 1;
    for (int blk = 0; blk <= R; ++blk) {
        const int t = block_table[blk];
        if (t < 0 || t >= num_tables) return MPQE_ERR_INVALID_ARG;
        if (!tables[t] || (uintptr_t)tables[t] % 16 != 0 || table_rows[t] < 1 || table_rows[t] > ((int64_t)1 << 40))
            return MPQE_ERR_INVALID_ARG;
        if (block_pad[blk] < 0 || block_pad[blk] >= table_rows[t]) return MPQE_ERR_INVALID_ARG;
        S->src[blk] = tables[t];
        S->src_rows[blk] = table_rows[t];
        S->pad[blk] = block_pad[blk];
        S->tab[blk] = t;
        if (table_rows[t] > max_rows) max_rows = table_rows[t];
    }
    if (B > 0 && (!self_rows || (R > 0 && (!neigh || !counts)))) return MPQE_ERR_INVALID_ARG;
    if (with_ws) {
        if (!workspace || (uintptr_t)workspace % 256 != 0) return MPQE_ERR_INVALID_ARG;
        if (workspace_bytes < L->total) return MPQE_ERR_WORKSPACE;
        char *wb = reinterpret_cast<char *>(workspace);
        S->feat = reinterpret_cast<float *>(wb + L->feat);
        S->z = reinterpret_cast<float *>(wb + L->z);
        S->stats = reinterpret_cast<float *>(wb + L->stats);
    }
    S->R = R;
    S->din = (int)din;
    S->dout = (int)dout;
    S->max_keep = max_keep;
    S->ln = gamma != nullptr;
    S->num_tables = num_tables;
    S->row_bits = bits_for((unsigned long long)(max_rows - 1));
    S->B = B;
    S->K = (long long)(R + 1) * din;
    S->neigh = reinterpret_cast<const long long *>(neigh);
    S->self_rows = reinterpret_cast<const long long *>(self_rows);
    S->counts = reinterpret_cast<const int *>(counts);
    S->W = W;
    S->gamma = gamma;
    S->beta = beta;
    S->eps = eps;
    S->err = err;
    return MPQE_OK;
}

extern "C" int mpqe_sage_fwd(const float *const *tables_host, const int64_t *table_rows_host, int num_tables,
                             const int32_t *block_table_host, const int64_t *block_pad_host, int num_rels,
                             const int64_t *neigh, const int32_t *counts, int max_keep, const int64_t *self_rows,
                             int64_t batch, const float *W, int64_t dim_in, int64_t dim_out, const float *gamma,
                             const float *beta, float eps, int save_states, float *out, void *workspace,
                             size_t workspace_bytes, int32_t *err, void *stream) {
    SageDev S;
    SageLayout L;
    const int st = sage_bind(tables_host, table_rows_host, num_tables, block_table_host, block_pad_host, num_rels, neigh, counts,
                             max_keep, self_rows, batch, W, dim_in, dim_out, gamma, beta, eps, workspace, workspace_bytes,
                             save_states != 0, err, &S, &L);
    if (st != MPQE_OK) return st;
    if (batch == 0) return MPQE_OK;
    if (!out || (uintptr_t)out % 16 != 0) return MPQE_ERR_INVALID_ARG;
    S.save = save_states != 0;
    hipLaunchKernelGGL(sage_fwd_kernel, dim3((unsigned)((batch + SG_ROWS - 1) / SG_ROWS)), dim3(256), 0, as_stream(stream), S,
                       out);
    return mpqe_launch_status();
}

extern "C" int mpqe_sage_bwd(const float *const *tables_host, const int64_t *table_rows_host, int num_tables,
                             const int32_t *block_table_host, const int64_t *block_pad_host, int num_rels,
                             const int64_t *neigh, const int32_t *counts, int max_keep, const int64_t *self_rows,
                             int64_t batch, const float *W, int64_t dim_in, int64_t dim_out, const float *gamma,
                             const float *beta, float eps, const float *out, const float *grad_out,
                             float *const *grad_tables_host, float *grad_W, float *grad_gamma, float *grad_beta,
                             void *workspace, size_t workspace_bytes, int32_t *err, void *stream) {
    SageDev S;
    SageLayout L;
    int st = sage_bind(tables_host, table_rows_host, num_tables, block_table_host, block_pad_host, num_rels, neigh, counts,
                       max_keep, self_rows, batch, W, dim_in, dim_out, gamma, beta, eps, workspace, workspace_bytes, true, err,
                       &S, &L);
    if (st != MPQE_OK) return st;
    bool any_table = false;
    if (grad_tables_host)
        for (int blk = 0; blk <= num_rels; ++blk) {
            S.gsrc[blk] = grad_tables_host[S.tab[blk]];
            if (S.gsrc[blk] && (uintptr_t)S.gsrc[blk] % 16 != 0) return MPQE_ERR_INVALID_ARG;
            any_table = any_table || S.gsrc[blk];
        }
    if (grad_W && (uintptr_t)grad_W % 16 != 0) return MPQE_ERR_INVALID_ARG;
    if (batch == 0) return MPQE_OK;
    if (!out || !grad_out || (uintptr_t)out % 16 != 0 || (uintptr_t)grad_out % 16 != 0) return MPQE_ERR_INVALID_ARG;
    const bool params = S.ln && (grad_gamma || grad_beta);
    if (!any_table && !grad_W && !params) return MPQE_OK;
    char *wb = reinterpret_cast<char *>(workspace);
    float *dz = reinterpret_cast<float *>(wb + L.dz), *gfeat = reinterpret_cast<float *>(wb + L.gfeat);
    float *dummy = reinterpret_cast<float *>(wb + L.dummy);
    const float *gz = grad_out;
    if (S.ln) {
        // (a gradient that is not wanted lands in scratch: the kernel forms both sums in one pass)
        st = mpqe_layernorm_relu_bwd(grad_out, S.z, out, batch, dim_out, gamma, S.stats, eps, 1, dz, grad_gamma ? grad_gamma : dummy,
                                     grad_beta ? grad_beta : dummy + dim_out, wb + L.ln_ws, L.ln_bytes, stream);
        if (st != MPQE_OK) return st;
        gz = dz;
    }
    if (!any_table && !grad_W) return MPQE_OK;
    // grad_W += gz^T . feat and g_feat = gz . W; without the normalisation the ReLU's mask is applied to grad_out here
    st = mpqe_linear_bwd(S.feat, batch, W, S.K, S.ln ? nullptr : out, gz, S.K, dim_out, S.ln ? 0 : 1, 0,
                         any_table ? gfeat : nullptr, grad_W, S.K, nullptr, wb + L.lin_ws, L.lin_bytes, stream);
    if (st != MPQE_OK || !any_table) return st;
    hipStream_t s = as_stream(stream);
    // (keys are long long, not the step's unsigned type: the sort's kernels are then this file's own instantiation)
    long long *keys_in = reinterpret_cast<long long *>(wb + L.keys_in);
    long long *keys_out = reinterpret_cast<long long *>(wb + L.keys_out);
    int *perm = reinterpret_cast<int *>(wb + L.perm);
    hipLaunchKernelGGL(sage_keys_kernel, dim3((unsigned)((L.n_ent + 255) / 256)), dim3(256), 0, s, S, L.n_ent, keys_in);
    const int key_bits = S.row_bits + bits_for((unsigned long long)num_tables);
    st = radix_sort_pairs_own<long long>(wb + L.sort_tmp, (const long long *)keys_in, keys_out, nullptr, perm, L.n_ent, key_bits, s);
    if (st != MPQE_OK) return st;
    hipLaunchKernelGGL(sage_rows_kernel, dim3((unsigned)((L.n_ent + 3) / 4)), dim3(256), 0, s, S, L.n_ent,
                       (const long long *)keys_out, (const int *)perm, (const float *)gfeat);
    return mpqe_launch_status();
}
