// The gradient reductions behind the mixed backwards (gqe_mixed_train.h, rgcn_mixed_train.h) and mpqe_gqe_bwd: ONE
// definition of every order of additions the bit-exactness tests pin. A model supplies what differs -- how its entries and
// contributions are reached -- as a small struct of __device__ __forceinline__ members handed over by value or reference;
// the kernels stay the models' own thin __global__ wrappers. No float atomics anywhere: every order below is a function
// of the call's indices alone, so the bits are the same every run.
//
// Stretches (mix_find_stretch): the rows of a call are cut into blocks and a block into its maximal stretches of rows
// with one formula; a workgroup owns the want-th stretch of its block and leaves at once when the block has fewer. The
// scan uses the block index and uniform loads only, so its result is wave-uniform.
//
// Table rows (rows_reduce): every looked-up row is an entry with a key (table index << 40 | row; -1: none). A wave per
// entry; the first entry of a key sums the key's entries in entry order -- per entry dv = (g - y (y . g)) / |v| with
// y = v / |v| the normalised table row -- and adds the sum to the table gradient: one writer per row.
//
// Parameters (mix_seg, param_reduce, vec_reduce): the contributions are sorted stably by parameter key (radix_sort.h),
// mix_seg finds every key's segment [first, end) of the sorted list, and a segment is cut into chunks of CHUNK
// consecutive contributions. A chunk is summed in list order from a zero accumulator, the chunk sums are added in chunk
// order, and the total is added to the caller's buffer by its one owner. Matrices (param_reduce): workgroup = (key, strip
// of 16 gradient rows), a chunk's outer products on v_mfma_f32_16x16x4_f32 with K = the contributions, lane group l >> 4
// feeding contribution c + (l >> 4); the chunk pass and the pass over the chunk sums are ONE launch (the workgroup that
// owns the strip walks the chunks, no partial matrices in memory) with the order two launches would have. Vectors
// (vec_reduce): the same with rows in place of outer products, one workgroup, a thread per column.
//
// Pairs (pair_cosine): the table row normalised in registers (row_norm_store's arithmetic, nothing stored), then
// cosine_fwd_kernel's three wave sums against the query row.
#pragma once
#include <new>

#include "gemm_core.h"

// the want-th maximal stretch [first, end) of one formula among rows [base, base + rows) below `limit` -> its formula
// (formula_of(row); -1: out of range), or false where the block has fewer stretches
template <typename FormulaOf>
__device__ __forceinline__ bool mix_find_stretch(long long base, int rows, long long limit, int want,
                                                 const FormulaOf &formula_of, long long &first, long long &end, int &fi) {
    int cnt = -1;
    long long prev = -2;
    first = end = base;
    fi = -1;
    for (int i = 0; i < rows; ++i) {
        const long long r = base + i;
        if (r >= limit) break;
        const long long k = formula_of(r);
        if (k != prev) {
            if (cnt == want) break;
            ++cnt;
            first = r;
            fi = (int)k;
            prev = k;
        }
        end = r + 1;
    }
    return cnt == want;
}

// Entries: keys() the entries' keys; tables(e, key, tab, gtab) the table entry e looked its row up in and that table's
// gradient buffer; grad_row(e) the gradient of entry e's normalised row
template <typename Entries>
__device__ __forceinline__ void rows_reduce(const Entries &E, long long n_ent, int D) {
    const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (e >= n_ent) return;
    const long long *keys = E.keys();
    const long long key = keys[e];
    if (key < 0) return;
    float earlier = 0.f;
    for (long long j0 = 0; j0 < e; j0 += 64) {
        const long long j = j0 + lane;
        if (j < e && keys[j] == key) earlier = 1.f;
    }
    if (wave_sum(earlier) > 0.f) return;
    const int c = lane * 4;
    const long long row = key & ((1ll << 40) - 1);
    const float *tab;
    float *gtab;
    E.tables(e, key, tab, gtab);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (c < D) v = gload4(tab + row * D + c);
    const float nrm = sqrtf(wave_sum(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]));
    const float inv = 1.f / nrm;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (long long j0 = e; j0 < n_ent; j0 += 64) {
        const long long j = j0 + lane;
        const float mine = (j < n_ent && keys[j] == key) ? 1.f : 0.f;
        if (!(wave_sum(mine) > 0.f)) continue;
        for (int l = 0; l < 64; ++l) {
            if (!(__shfl(mine, l, 64) > 0.f)) continue;
            const float *gr = E.grad_row(j0 + l);
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
            if (c < D) g = gload4(gr + c);
            const float ydotg = wave_sum(v[0] * g[0] + v[1] * g[1] + v[2] * g[2] + v[3] * g[3]) * inv;
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] += (g[u] - (v[u] / nrm) * ydotg) * inv;
        }
    }
    if (c < D) {
        float *o = gtab + row * D + c;
        f32x4 old = *reinterpret_cast<const f32x4 *>(o);
#pragma unroll
        for (int u = 0; u < 4; ++u) old[u] += acc[u];
        *reinterpret_cast<f32x4 *>(o) = old;
    }
}

// seg[k] = [first, end) of key k < nkeys in the sorted list of NC keys (cleared before); a thread per list position
__device__ __forceinline__ void mix_seg(const unsigned *skey, int *seg, long long NC, unsigned nkeys) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= NC) return;
    const unsigned k = skey[i];
    if (k >= nkeys) return;
    if (i == 0 || skey[i - 1] != k) seg[2 * k] = (int)i;
    if (i == NC - 1 || skey[i + 1] != k) seg[2 * k + 1] = (int)(i + 1);
}

// strip rs of the [D, D] matrix g += the outer products of segment [lo, hi) of sval; Contrib::rows(value, A, B): the rows
// that feed the MFMA's A and B operand
template <int CHUNK, typename Contrib>
__device__ __forceinline__ void param_reduce(int lo, int hi, int rs, float *g, int D, const int *sval, const Contrib &C) {
    const int nstrip = D / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, kq = lane >> 4;
    if (wave >= nstrip) return;
    f32x4 tot[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) tot[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = lo; c0 < hi; c0 += CHUNK) {
        const int ce = c0 + CHUNK < hi ? c0 + CHUNK : hi;
        f32x4 acc[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c = c0; c < ce; c += 4) {
            // lane group kq feeds contribution c + kq (past the chunk: zeros)
            float a = 0.f, b[4] = {0.f, 0.f, 0.f, 0.f};
            if (c + kq < ce) {
                const float *A, *Bp;
                C.rows((unsigned)sval[c + kq], A, Bp);
                a = gload1(A + 16 * rs + j);
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if (wave + 4 * m < nstrip) b[m] = gload1(Bp + 16 * (wave + 4 * m) + j);
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (wave + 4 * m < nstrip) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[m], acc[m], 0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) tot[m][r] += acc[m][r];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (wave + 4 * m >= nstrip) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) g[(long long)(16 * rs + 4 * kq + r) * D + 16 * (wave + 4 * m) + j] += tot[m][r];
    }
}

// the [D] vector g += the rows of segment [lo, hi) of sval; Contrib::term(value): the row a contribution adds
template <int CHUNK, typename Contrib>
__device__ __forceinline__ void vec_reduce(int lo, int hi, float *g, int D, const int *sval, const Contrib &C) {
    if ((int)threadIdx.x >= D) return;
    float tot = 0.f;
    for (int c0 = lo; c0 < hi; c0 += CHUNK) {
        const int ce = c0 + CHUNK < hi ? c0 + CHUNK : hi;
        float acc = 0.f;
        for (int c = c0; c < ce; ++c) acc += gload1(C.term((unsigned)sval[c]) + threadIdx.x);
        tot += acc;
    }
    g[threadIdx.x] += tot;
}

// one pair by one wave: row `row` of `tab` (< 0, a bad id: zeros, not read) normalised against the query row qi
struct PairCosine {
    float dot, qq, tt, nrm;     // q . t, q . q, t . t over the normalised row t = v / nrm
};
__device__ __forceinline__ PairCosine pair_cosine(const float *qi, const float *tab, long long row, int D, int lane) {
    const float *v = tab + (row < 0 ? 0 : row) * D;
    PairCosine p = {0.f, 0.f, 0.f, 1.f};
    if (row >= 0) {
        float ss = 0.f;
        for (int c = lane * 4; c < D; c += 256) {
            const f32x4 u = gload4(v + c);
            ss += u[0] * u[0] + u[1] * u[1] + u[2] * u[2] + u[3] * u[3];
        }
        ss = wave_sum(ss);
        p.nrm = sqrtf(ss);
    }
    for (int c = lane; c < D; c += 64) {
        const float a = gload1(qi + c);
        float b = 0.f;
        if (row >= 0) b = gload1(v + c) / p.nrm;
        p.dot += a * b;
        p.qq += a * a;
        p.tt += b * b;
    }
    p.dot = wave_sum(p.dot);
    p.qq = wave_sum(p.qq);
    p.tt = wave_sum(p.tt);
    return p;
}

// ------------------------------------------------------------------------------------------------ host side
// a host image of `count` T, filled by fill(image) -> status, to device memory in one copy
template <typename T, typename Fill>
static int mix_upload(void *dst, size_t count, hipStream_t s, Fill fill) {
    T *image = new (std::nothrow) T[count];
    if (!image) return MPQE_ERR_INVALID_ARG;
    int st = fill(image);
    if (st == MPQE_OK && hipMemcpyAsync(dst, image, count * sizeof(T), hipMemcpyHostToDevice, s) != hipSuccess)
        st = MPQE_ERR_LAUNCH;
    // (the copy reads pageable memory: it has left `image` when the call returns)
    delete[] image;
    return st;
}

// the caller's `np` gradient buffers' addresses (NULL: not wanted), every one 16-byte aligned
template <typename Fill>
static int mix_upload_grad_ptrs(void *dst, size_t np, hipStream_t s, Fill fill) {
    return mix_upload<float *>(dst, np, s, [&](float **image) -> int {
        fill(image);
        for (size_t k = 0; k < np; ++k)
            if ((uintptr_t)image[k] % 16 != 0) return MPQE_ERR_INVALID_ARG;
        return MPQE_OK;
    });
}
