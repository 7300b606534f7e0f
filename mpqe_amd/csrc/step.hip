// Fused training step: forward + backward of the whole query-graph encoder for ALL batches of
// one step (the reference's post-burn-in step draws 11 formula batches: train_helpers.py:81,
// 97-112; each goes through RGCNEncoderDecoder.margin_loss, model.py:464-494) in ~15 kernel
// launches instead of one launch per op per batch.
//
// At the reference's batch size (B = 512, <= 4 nodes per graph, D = 128) every single op is
// far too small to fill 256 CUs and the path is launch-latency bound. So the unit of a launch
// here is a LEVEL of the whole step: level p applies message-passing pass p of every batch
// that still has a pass to run (batches differ in template, relations and number of passes),
// as one grid of 64x64 MFMA tiles described by a small descriptor table in HBM.
//
//   forward   assemble (anchors: gather + L2 normalise; variables: mode rows; +/- targets)
//             level 0 .. Lmax-1 layer tiles
//             readout + cosine(+/-) + hinge terms per graph;  loss reduction (one workgroup)
//   backward  d hinge -> d cosine -> d readout -> rows of gH[L_b]; target/negative table grads
//             level Lmax-1 .. 0 backward-x tiles
//             weight-gradient tiles of ALL levels (split over K chunks, slabs)
//             bias / variable-row partial sums; anchor table grads
//             one reduction pass: slabs and partials -> gradients, fixed order
//
// Arithmetic is identical to the per-op kernels (same tile bodies, rgcn_template_body.h);
// margin_loss's two encoder passes are one here (the query embedding does not depend on the
// target).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "grad_w_dma.h"
#include "rgcn_template_body.h"

#define STEP_MAX_LEVELS MPQE_STEP_MAX_LAYERS
#define CHAIN_MAX_GRAPHS (1 << 20)
#define UPLOAD_BYTES 2048

struct BatchDev {
    TmplArgs tp;
    int A, V, L, B;
    long long var_id[3];
    int anchor_tab[3];
    int target_tab;
    long long row_off, g_off, anchor_off;
    float weight;
    int pad;
    // live[p]: node slots whose state H[p] can reach the readout (bit n). Everything else is neither
    // computed nor read: its gradient is exactly zero (MPQE_STEP_NO_PRUNE: all slots at every level).
    unsigned live[MPQE_STEP_MAX_LAYERS + 1];
    int pad2;
    // chain form. uvL[n] >= 0: node slot n is still batch-uniform at level L; its state is the pre-pass vector with that
    // granule slot (the readout reads it in every row). lpart[n] >= 0: first row in `parts` of the per-block column sums of
    // gH[L][n] (row = lpart[n] + block index inside the batch).
    int uvL[4], lpart[4];
};

struct StepDev {
    int nb, D, num_layers, readout;
    long long rows_total, graphs_total;
    BatchDev b[MPQE_STEP_MAX_BATCHES];
};

struct LayerPtrs {
    const float *basis[MPQE_STEP_MAX_LAYERS], *root[MPQE_STEP_MAX_LAYERS], *bias[MPQE_STEP_MAX_LAYERS];
};
struct TablePtrs {
    const float *table[MPQE_STEP_MAX_MODES];
    float *grad[MPQE_STEP_MAX_MODES];
    long long rows[MPQE_STEP_MAX_MODES];
};

// Tiles of one (batch, node slot) at one level: rt*ct tiles of equal K length. Per-CU MFMA time is
// what bounds a level, and a level's workgroups are (almost always) all resident at once, dealt
// round-robin over the 256 CUs: block i shares its CU with blocks i+256, i+512, i+768 (measured,
// tools/micro/placement.hip; a speed assumption only, results do not depend on it). place_tiles() orders
// the table so that those per-CU sums are balanced (longest-processing-time-first bin packing).
struct TileGroup {
    int batch, node, tile_off, steps;
};
// One entry per workgroup of a level launch: a workgroup finds its work with ONE 8-byte load instead
// of a binary search over the groups (each probe is a dependent ~0.5 us scalar round trip that sits in
// front of the first MFMA; with launches this short that start-up cost is a visible share).
struct TileRef {
    short batch, node;
    int rem;            // tile index inside the (batch, node) group: row tile * ct + column tile
};

// one weight-gradient source: (batch, level, slot) -> nch K-chunks, each a slab of D*D floats
// one weight-gradient workgroup, everything it needs in one 64-byte record (the host resolved source, batch
// and template: three dependent loads in front of the first DMA otherwise)
struct WBlock {
    long long x_off, g_off;     // float offsets into H / gH: level base + the batch's first row
    long long slab_off;         // float offset of the chunk's slab
    long long rel;              // direct: relation id (-1 = root)
    int xs, xo, go;             // rows of graph q: x at (q * xs + xo), g at (q * xs + go)
    int q0, q1;                 // the K-chunk: graphs [q0, q1)
    int i0, j0;                 // the output tile
    int direct;                 // >= 0: layer whose gradient matrix the tile writes itself; -1: slab
    int d0, dn;                 // merged launch: the `done` counters [d0, d0 + dn) cover the chain workgroups of the K-chunk
    int batch, pad;             // pad = 1: the operands change places -- x rows from gH (at g_off), g rows from H (at x_off): the
                                // tile is then the gradient of an nn.Linear weight [out, in] (a learned readout on the chain)
};
// Merged launch (chain form): the weight-gradient tiles and the backward post-pass are workgroups of the CHAIN launch,
// behind the chain workgroups. A chain workgroup counts itself into the `done` counter of its group of DONE_GRAPHS graphs
// once its H / gH rows and column sums are out (release at agent scope); a tile / vector op waits for the counters of
// the graphs it reads. Counters only grow: target = (merged-launch epoch + 1) x (chain workgroups of the group).
#define STEP_XCDS_MAX 8
#define DONE_GRAPHS 128
struct DoneMeta {
    int base[MPQE_STEP_MAX_BATCHES + 1];       // counters of batch b: [base[b], base[b + 1])
};
struct WSource {
    int batch, level, slot, relu;
    int nch, ch, slab_start, block_start;
    // direct >= 0: this source is the ONLY contribution to its gradient matrix and one K-chunk: the tile adds
    // straight into the gradient (layer `direct`, relation `rel`, -1 = root), no slab, no reduction group
    int direct, pad;
    long long rel;
};
// one partial-vector source: kind 0 = bias colsum of (batch, level), kind 1 = variable row (batch, k)
struct VSource {
    int kind, batch, level_or_k, relu;
    int nblk, part_start, block_start, pad;
};
// one reduction group: out[...] += sum of `count` consecutive slabs/partials starting at `start`
// (+ matrices, chain form with uniform node states: the sum of r1_count rank-1 terms u (x) v from `r1_start` on)
struct RGroup {
    int kind;          // 0 basis, 1 root, 2 bias, 3 mode row; 4: a D x D column block of a [D, n D] matrix (`root` of `layer`:
                       // a learned readout's first Linear layer), row = block | n << 8
    int layer;         // layer index (kinds 0-2)
    long long row;     // relation id (kind 0) / mode id (kind 3)
    int start, count;
    int r1_start, r1_count;
};
struct Rank1 {
    int u, v;          // vector ids: out[i][j] += VT[u][i] * VT[v][j]
};
#ifndef R1_CHUNK
#define R1_CHUNK 8
#endif
#ifndef STEP_DBG
#define STEP_DBG 0      // timing experiments only (wrong results): 1 = no table-sum rows in the reduction launch,
#endif                  // 2 = no rank-1 terms, 3 = neither

// ---- batch-uniform node states (chain form; include/mpqe_amd.h: MPQE_STEP_NO_UNIFORM) --------------------------
// x0's variable rows are ONE mode_embeddings row for every graph of a batch (reference model.py:421), so a node state
// that no anchor has reached yet is one vector per batch. Per batch and level p the node slots split into uniform
// (U) and per-graph (NU) ones: U[0] = the variable slots, n in U[p+1] iff n and all sources of its in-edges are in
// U[p]. Consequences, all exact:
//   forward   a U node update is a matrix-VECTOR product chain, done once per batch (UOP_FWD, pre-pass, rides in the
//             prologue launch). An NU node's U sources add a constant vector to its pre-activation: the pre-pass
//             forms bias + that constant, the chain kernel's epilogue adds it where it added the bias.
//   backward  everything downstream of a U node's gradient needs only its COLUMN SUM over the batch (its inputs
//             are uniform, so its weight gradients are rank-1: u (x) colsum; its ReLU mask is uniform, so masking
//             commutes with the sum; bias / variable-row gradients are column sums anyway). The chain kernel leaves
//             per-block column sums of every NU node's gradient rows in `parts`; the post-pass (rides in the
//             weight-gradient launch) sums them over the blocks (UOP_RED) and runs the U nodes' backward as
//             vector-matrix^T products on those sums (UOP_BWD).
// Vectors live in the vector table VT [id][D] of the workspace; vectors that are handed from one workgroup to
// another INSIDE a launch also travel as {tag, value} granules (8 bytes, one agent-scope atomic store each: the data
// is its own flag -- MI355X guide, inter-workgroup visibility, form R2) in the packed step's descriptor buffer.
#define UOP_FWD 0      // out = act(bias[layer] + sum_t in_t . M_t)
#define UOP_BWD 1      // out = mask(VT[mask_vec] > 0) * sum_t in_t . M_t^T
#define UOP_RED 2      // out = sum of `nrows` consecutive rows of `parts` from row0
#define UOP_COPY 3     // out = mode_emb[mode_row]
#define UOP_R1 4       // gradient matrix (layer r1_layer, relation r1_rel | -1 root) = sum_t VT[u_vec[t]] (x) in_t: a matrix
                       // whose only contributions are rank-1 terms is written here, not by the reduction launch
#define UOP_MAX_TERMS 4
struct UOp {
    int kind, out_vec, out_gran;       // out_gran: granule slot of the output (-1: nobody reads it inside the launch)
    int out_part;                      // >= 0: the output is also written to this row of `parts` (a reduction group's input)
    int nterms;
    int in_vec[UOP_MAX_TERMS];         // vector id (in_kind 0: read from its granules; 2: plain, written by an earlier launch)
    int in_kind[UOP_MAX_TERMS];        // 0 granules, 1 row in_vec of mode_emb, 2 plain VT, 3 sum of in_gran rows of `parts` from row in_vec
    int in_gran[UOP_MAX_TERMS];
    int layer[UOP_MAX_TERMS], mat[UOP_MAX_TERMS];      // matrix: relation id or -1 = root, of layer `layer`
    int bias_layer, relu;              // FWD
    int mask_vec;                      // BWD: -1 = no mask
    int row0, nrows;                   // RED
    long long mode_row;                // COPY
    int u_vec[UOP_MAX_TERMS];          // R1
    int r1_layer, r1_rel;
    unsigned wait_mask;                // merged launch: bit b = the op reads rows the chain workgroups of batch b write
};

struct Blob {
    char bytes[UPLOAD_BYTES];
};
__global__ void step_upload_kernel(Blob blob, char *dst, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = blob.bytes[i];
}

__device__ __forceinline__ int find_le(const int *__restrict__ off, int n, int t) {
    // largest i in [0, n) with off[i] <= t   (off non-decreasing, off[0] = 0)
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// lp.X[li] with a runtime li would spill the by-value pointer table to scratch; select instead
__device__ __forceinline__ const float *pick_layer(const float *const *arr, int li) {
    const float *r = arr[0];
#pragma unroll
    for (int l = 1; l < MPQE_STEP_MAX_LAYERS; ++l)
        if (l == li) r = arr[l];
    return r;
}

__device__ __forceinline__ int find_group_le(const TileGroup *__restrict__ g, int n, int t) {
    int lo = 0, hi = n - 1;     // largest i in [0, n) with g[i].tile_off <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (g[mid].tile_off <= t) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int layer_index(int p, int L, int num_layers) {
    return p < L - 1 ? p : num_layers - 1;     // reference model.py:435-441
}

// ------------------------------------------------------------------------------------ assemble
__device__ __forceinline__ long long table_row(const long long *__restrict__ node_map, long long map_len,
                                               long long id, long long rows, int32_t *err) {
    if (id < 0 || id >= map_len) {
        flag_error(err, MPQE_FLAG_BAD_NODE_ID);
        return -1;
    }
    const long long r = node_map[id];
    if (r < 0 || r >= rows) {
        flag_error(err, MPQE_FLAG_BAD_NODE_ID);
        return -1;
    }
    return r;
}

struct GradPtrs {
    float *basis[MPQE_STEP_MAX_LAYERS], *root[MPQE_STEP_MAX_LAYERS], *bias[MPQE_STEP_MAX_LAYERS];
    float *mode_emb;
};
__device__ __forceinline__ float *pick_grad(float *const *arr, int li) {
    float *r = arr[0];
#pragma unroll
    for (int l = 1; l < MPQE_STEP_MAX_LAYERS; ++l)
        if (l == li) r = arr[l];
    return r;
}

#include "step_chain.h"
#include "step_uniform.h"
#include "step_touch.h"
#include "grad_w_reg.h"
#include "step_readout.h"
#define LD_T 3          // weight-gradient launch of the chain form: register-only K loop (grad_w_reg.h)

// Prologue roles of the chain launch (they were a launch of their own, 9 us in front of the chain kernel): the forward
// pre-pass of the batch-uniform node states (vector ops, step_uniform.h), transposed copies of the matrices the backward
// chains multiply by (64 x 64 pieces through LDS), zero fill of the gradient buffers (MPQE_STEP_ZERO_GRADS).
struct WtSlot {
    int layer, mat;       // mat < 0: root
    // a learned readout's first Linear layer may be WIDE (targetmlp: [D, 2 D]): the copy is of its D x D column block from
    // column col0 on, row length ld; plain: copied as it is (the backward chains multiply by the block itself), not transposed
    int col0, ld, plain;
};
#define PREP_MAX_SEGS 48
struct ZeroSegs {
    float *p[PREP_MAX_SEGS];
    long long n[PREP_MAX_SEGS];       // floats
    long long block0[PREP_MAX_SEGS + 1];   // first zero-fill workgroup of each segment
    int count;
};
#define PREP_ZERO_FLOATS_PER_BLOCK 8192      // 256 threads x 8 x float4
// Chain form: every chain block left the sum of its (<= 16) hinge terms in block_terms, and everything the
// reduction needs to know about the batches comes by value -- no dependent loads in front of the sums.
struct LossMeta {
    int nb, chain;
    int B[MPQE_STEP_MAX_BATCHES], blk_off[MPQE_STEP_MAX_BATCHES + 1];
    float weight[MPQE_STEP_MAX_BATCHES];
};
__device__ __forceinline__ void loss_block_chain(const LossMeta &lm, const float *__restrict__ bterms,
                                                 float *__restrict__ loss, float *mean, int nwaves) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int bi = w; bi < lm.nb; bi += nwaves) {
        float s = 0.f;
        for (int i = lm.blk_off[bi] + lane; i < lm.blk_off[bi + 1]; i += 64) s += bterms[i];
        s = wave_sum(s);
        if (lane == 0) {
            mean[bi] = s / (float)lm.B[bi];
            loss[1 + bi] = mean[bi];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.f;
        for (int bi = 0; bi < lm.nb; ++bi) total += lm.weight[bi] * mean[bi];
        loss[0] = total;
    }
}

// Forward-only step in the chain form: the loss reduction, the epoch advance and the caller's notification ride in the chain
// launch itself -- every workgroup of the launch counts itself out as it ends, and the LAST one to end does what
// step_loss_kernel does as a launch of its own (one launch per margin_loss call of the drop-in entry points instead of two:
// ~2.5 us of host time and ~6 us of device time per call). The chain workgroups' block_terms are written through
// (agent-scope stores, acknowledged before the count) and read back the same way: no L2 write-back.
struct FinArgs {
    unsigned *count;          // workgroups of this launch that have ended (the last one leaves 0 behind); NULL: not this form
    float *loss;
    const float *bterms;
    unsigned *epoch_f;
    int bump_b;
    unsigned *notify;
    unsigned notify_value;
    const int32_t *err;
    const float *reg_norms;   // != NULL: loss[0] += reg_coef * *reg_norms (mpqe_step_extra_t.readout_norms: the readout's regulariser)
    float reg_coef;
    LossMeta lm;
};
__device__ __forceinline__ void chain_finish(const FinArgs &fin, float *smem) {
    __syncthreads();          // (every wave is through its role: the state buffers are free)
    unsigned *flag = reinterpret_cast<unsigned *>(smem);
    float *mean = smem + 16;
    if (threadIdx.x == 0) {
#ifndef MPQE_EMU
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (this thread's block_terms store has been acknowledged)
#endif
        *flag = atomicAdd(fin.count, 1u) + 1u == gridDim.x ? 1u : 0u;
    }
    __syncthreads();
    if (*flag == 0u) return;
    const LossMeta &lm = fin.lm;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = (int)(blockDim.x >> 6);
    for (int bi = w; bi < lm.nb; bi += nwaves) {              // (step_loss_kernel's sums, term for term)
        float s = 0.f;
        for (int i = lm.blk_off[bi] + lane; i < lm.blk_off[bi + 1]; i += 64)
            s += agent_load(fin.bterms + i);
        s = wave_sum(s);
        if (lane == 0) {
            mean[bi] = s / (float)lm.B[bi];
            fin.loss[1 + bi] = mean[bi];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.f;
        for (int bi = 0; bi < lm.nb; ++bi) total += lm.weight[bi] * mean[bi];
        // (step_ro_reg_kernel's `loss[0] = fma(coef, sum of the norms, loss[0])`, with the norms of mpqe_step_readout_norms)
        if (fin.reg_norms) total = __builtin_fmaf(fin.reg_coef, *fin.reg_norms, total);
        fin.loss[0] = total;
        agent_store(fin.count, 0u);
        // (the next step's forward granules get a new tag, step_uniform.h; the transposed copies' count a new target)
        *fin.epoch_f = *fin.epoch_f + 1u;
        if (fin.bump_b) *(fin.epoch_f + 16) = *(fin.epoch_f + 16) + 1u;
        if (fin.notify) {
            fin.notify[1] = fin.err ? (unsigned)agent_load(fin.err) : 0u;
#ifndef MPQE_EMU
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");        // (system scope: the flags word is out before the number)
#endif
            fin.notify[0] = fin.notify_value;
        }
    }
}

struct PrepArgs {
    UArgs ua;
    TSortArgs ts;             // the touch plan's sort (MPQE_STEP_BUILD_TOUCH): workgroups [0, sblocks) of the launch --
    int sblocks;              // dealt to the XCDs of `sxrank` only (4 bits per XCD: rank + 1, 0 = none; workgroup b of a
    int sna;                  // launch runs on XCD b % 8): the first sblocks = 8 x rows workgroups of the launch are ROWS of
    unsigned sxrank;          // eight -- the sort's XCDs take sort workgroups, the others go on with the prologue's items
    int strail;               // != 0: the launch's LAST strail workgroups instead (diagnostics switch TSORT_TRAIL)
    int late;                 // diagnostics ("HANDOFF_LATE"): the first transpose workgroup counts itself in ~1 s late -- a producer
                              // that lost its CU to another process: its consumers' bounded waits run out (MPQE_FLAG_INTERNAL)
    int *runs_count;          // the number of run starts the weight-gradient launch will compact (touch_runs_block), zeroed here; or NULL
    int ublocks, tblocks;     // vector-op workgroups, transpose workgroups
    int lead;                 // prologue workgroups in front of the chain workgroups: sblocks + ublocks + tblocks rounded
                              // up to a multiple of 8 (chain workgroup b keeps XCD b % 8)
    int nchain;               // chain workgroups (holes of the placement grid included)
    int plast;                // != 0: the prologue's items BEHIND the chain workgroups ([sort rows][chain][items]). A prologue
                              // of more than one workgroup per CU holds slots the chain workgroups are dealt into: those wait
                              // until prologue workgroups end, here and there, and pair up on some CUs while others stay
                              // empty (AIFB step with the MLP readout, ~400 prologue workgroups: 203 of 256 CUs used, chain
                              // launch 172 us; behind the chain: 256 CUs, 133 us. The default step's ~230 fit beside the chain
                              // workgroups and are 1.2 us faster in front). Only when every chain workgroup is resident with
                              // slots to spare: a producer must never wait for a slot held by its consumers
    int plna;                 // ... and those items are dealt only to the plna XCDs whose CUs hold at most ONE chain workgroup
    unsigned plxrank;         // (4 bits per XCD: rank + 1, 0 = none): an XCD whose slots are all taken by chain workgroups
                              // would queue a producer behind its waiting consumers
    const WtSlot *slots;
    float *WT;
    unsigned *wt_count;
    // forward-only step with a learned readout: only the copies its forward multiplies by (tsel_n of them, slots tsel[]) are
    // made; the first transpose workgroup counts the tskip workgroups of the others in as well, so that the count advances
    // by the same number in every launch of the packed step (the chain workgroups' target: epoch x all)
    int tsel_n, tsel[8];
    unsigned tskip;
    unsigned *fwd_done;       // vector-op workgroups finished, ever (uop_wait_prepass); NULL: none
    ZeroSegs zs;
};

// one 64 x 64 piece of a matrix, transposed: T[c][r] = W[r][c] (D % 64 == 0 in the chain form)
__device__ __forceinline__ void prep_transpose_block(const LayerPtrs &lp, const PrepArgs &pa, int D, int tb, float *smem) {
    float(*tile)[65] = reinterpret_cast<float(*)[65]>(smem);
    const int tpd = D / 64, per = tpd * tpd;
    const int si = pa.tsel_n ? pa.tsel[tb / per] : tb / per, tr = (tb % per) / tpd, tc = tb % tpd;
    const WtSlot sl = pa.slots[si];
    const float *W = (sl.mat >= 0 ? pick_layer(lp.basis, sl.layer) + (long long)sl.mat * D * D : pick_layer(lp.root, sl.layer)) + sl.col0;
    const int ld = sl.ld;
    float *T = pa.WT + (long long)si * D * D;
    const int tid = threadIdx.x;
    if (tid < 256) {
        const int c4 = tid & 15, r0 = tid >> 4;               // 16 float4 columns x 16 rows per pass
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + 16 * q;
            const f32x4 v = gload4(W + (long long)(tr * 64 + r) * ld + tc * 64 + 4 * c4);
            if (sl.plain) *reinterpret_cast<f32x4 *>(T + (long long)(tr * 64 + r) * D + tc * 64 + 4 * c4) = v;
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[r][4 * c4 + e] = v[e];
        }
    }
    __syncthreads();
    if (tid < 256 && !sl.plain) {
        const int c4 = tid & 15, r0 = tid >> 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + 16 * q;                        // row of T = column of W
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = tile[4 * c4 + e][r];
            *reinterpret_cast<f32x4 *>(T + (long long)(tc * 64 + r) * D + tr * 64 + 4 * c4) = v;
        }
    }
    // publish: every storing wave drains its stores, the workgroup meets, ONE lane releases at agent scope and
    // counts the workgroup in (the consumers: chain_block, before the backward levels)
#ifndef MPQE_EMU
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    __syncthreads();
    if (tid == 0) {
#ifndef MPQE_EMU
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        atomicAdd(pa.wt_count, tb == 0 ? 1u + pa.tskip : 1u);
    }
}

__device__ __forceinline__ void prep_zero_block(const ZeroSegs &zs, long long zb) {
    if (threadIdx.x >= 256) return;
    int sg = 0;
    for (int i = 1; i < zs.count; ++i)
        if (zs.block0[i] <= zb) sg = i;
    const long long base = (zb - zs.block0[sg]) * PREP_ZERO_FLOATS_PER_BLOCK;
    float *p = zs.p[0];
    long long n = zs.n[0];
#pragma unroll
    for (int i = 1; i < PREP_MAX_SEGS; ++i)       // (a runtime index into the by-value table would spill it)
        if (i == sg) {
            p = zs.p[i];
            n = zs.n[i];
        }
    if (((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long i = base + (long long)(threadIdx.x + 256 * k) * 4;
            if (i + 3 < n) *reinterpret_cast<f32x4 *>(p + i) = f32x4{0.f, 0.f, 0.f, 0.f};
            else
                for (long long q = i; q < n; ++q) p[q] = 0.f;
        }
    } else {
        for (long long i = base + threadIdx.x; i < base + PREP_ZERO_FLOATS_PER_BLOCK && i < n; i += 256) p[i] = 0.f;
    }
}

// Merged launch: what used to be the weight-gradient launch -- zero fill of untouched relation matrices, the backward
// post-pass of the uniform node states, the weight-gradient tiles -- as workgroups of the chain launch, behind its zero
// fill: [prologue][chain][zero fill, padded to a multiple of 8][untouched matrices | post-pass, padded][tiles].
// They wait for the chain workgroups whose rows they read (DoneMeta) and for nothing that comes after them in the
// launch; with in-order dispatch per XCD every wait ends (and is bounded all the same).
struct ZMat {
    int layer, pad;
    long long rel;
};
#define ZMAT_FLOATS_PER_BLOCK 8192
struct WBlock;
struct PostArgs {
    int zpad;                 // zero-fill workgroups, padding included: the post roles start at lead + nchain + zpad; 0 = none
    int zmblocks, ublocks;    // untouched-matrix workgroups, post-pass workgroups
    int ppad;                 // zmblocks + ublocks rounded up to a multiple of na
    int na;                   // XCDs the post roles are dealt to; xrank: 4 bits per XCD, rank + 1 (0 = none)
    unsigned xrank;
    int wblocks, zper, D, zeroed;
    int tile_n;               // columns per weight-gradient tile
    UArgs ub;
    const WBlock *wblock;
    const ZMat *zmats;
    float *slabs;
    const float *H, *GH;
    long long level_stride;
    GradPtrs gp;
    const unsigned *done;
    const int *done_inc;
    const unsigned *epoch_m;  // epoch of the merged launches of this packed step (bumped by the reduction launch)
    int32_t *err;
    long long *stamps;        // diagnostics (mpqe_debug_tail_stamps): 8 words per tile workgroup, or NULL
};
template <int LDS_TILES>
__device__ __forceinline__ void post_block(const StepDev *__restrict__ sd, const LayerPtrs &lp, const PostArgs &po, int pb,
                                           float *smem);
__device__ __forceinline__ void zmat_block(const ZMat *__restrict__ zmats, int zper, int zb, int D, const GradPtrs &gp);

template <int NCB, int KS, int NW = 4, bool RO = false>
__global__ __launch_bounds__(64 * NW) void step_chain_kernel(const StepDev *__restrict__ sd, LayerPtrs lp,
                                                             TablePtrs tabs, ChainArgs ca, PrepArgs pa, PostArgs po) {
    __shared__ __attribute__((aligned(16))) ChainLds<NCB, KS, NW> S;
#define CHAIN_ROLES_RETURN return
#include "step_chain_roles.h"
#undef CHAIN_ROLES_RETURN
}
// ... and the forward-only step's instance, which ends with chain_finish (an instance of its own: the whole step's kernel
// keeps its arguments and its code as they were)
template <int NCB, int KS, int NW = 4, bool RO = false>
__global__ __launch_bounds__(64 * NW) void step_chain_fwd_kernel(const StepDev *__restrict__ sd, LayerPtrs lp,
                                                                 TablePtrs tabs, ChainArgs ca, PrepArgs pa, PostArgs po,
                                                                 FinArgs fin) {
    __shared__ __attribute__((aligned(16))) ChainLds<NCB, KS, NW> S;
#define CHAIN_ROLES_RETURN goto roles_done
#include "step_chain_roles.h"
#undef CHAIN_ROLES_RETURN
roles_done:
    chain_finish(fin, reinterpret_cast<float *>(&S));
}

// level form: zero fill of the gradient buffers (MPQE_STEP_ZERO_GRADS) as a launch of its own
__global__ __launch_bounds__(256) void step_zero_kernel(ZeroSegs zs) { prep_zero_block(zs, (long long)blockIdx.x); }

// rows [0, rows_total) are node rows of H0, then G positive and G negative targets. D/4 adjacent lanes
// own a row (two rows per wave at D = 128): the kernel is a chain of dependent gathers (id -> LUT ->
// table row), so more rows in flight per wave is what shortens it.
__global__ __launch_bounds__(256) void step_assemble_kernel(
    const StepDev *__restrict__ sd, TablePtrs tabs, const long long *__restrict__ node_map, long long map_len,
    const float *__restrict__ mode_emb, long long num_modes, const long long *__restrict__ anchor_ids,
    const long long *__restrict__ targets, const long long *__restrict__ negs, float *__restrict__ H0,
    float *__restrict__ tpos, float *__restrict__ tneg, int32_t *err, int vec, long long row0, long long R,
    long long g0, long long G) {
    // this launch covers node rows [row0, row0 + R) and graphs [g0, g0 + G) (one stream lane of the step)
    const int D = sd->D;
    const int lpr = lanes_per_row(D, vec), rpw = 64 / lpr;
    const int lane = threadIdx.x & 63, sub = lane & (lpr - 1);
    const long long wl = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + lane / lpr;
    // no early return: every lane takes part in the sub-wave shuffles; out-of-range groups idle
    const bool live = wl < R + 2 * G;
    const long long w = row0 + wl;        // global node row when wl < R
    int32_t *e = sub == 0 ? err : nullptr;
    const float *src = nullptr;
    float *dst = nullptr;
    bool normalise = true;
    if (live && wl < R) {
        int bi = 0;
        for (int i = 1; i < sd->nb; ++i)
            if (sd->b[i].row_off <= w) bi = i;
        const BatchDev &b = sd->b[bi];
        const long long lr = w - b.row_off;
        const long long g = lr / b.tp.N;
        const int n = (int)(lr - g * b.tp.N);
        dst = H0 + w * D;
        if (n < b.A) {
            const int tab = b.anchor_tab[n];
            const long long id = anchor_ids[b.anchor_off + (long long)n * b.B + g];
            const long long row = table_row(node_map, map_len, id, tabs.rows[tab], e);
            if (row >= 0) src = tabs.table[tab] + row * D;
        } else {
            const long long m = b.var_id[n - b.A];
            normalise = false;
            if (m < 0 || m >= num_modes) flag_error(e, MPQE_FLAG_BAD_NODE_ID);
            else src = mode_emb + m * D;
        }
    } else if (live) {
        const long long gi = g0 + (wl - R) % G;
        const bool is_neg = (wl - R) >= G;
        int bi = 0;
        for (int i = 1; i < sd->nb; ++i)
            if (sd->b[i].g_off <= gi) bi = i;
        const int tab = sd->b[bi].target_tab;
        const long long id = is_neg ? negs[gi] : targets[gi];
        const long long row = table_row(node_map, map_len, id, tabs.rows[tab], e);
        if (row >= 0) src = tabs.table[tab] + row * D;
        dst = (is_neg ? tneg : tpos) + gi * D;
    }
    if (live && (!src || !normalise)) {
        if (vec) {
            for (int c = sub * 4; c < D; c += 4 * lpr)
                *reinterpret_cast<f32x4 *>(dst + c) = src ? *reinterpret_cast<const f32x4 *>(src + c)
                                                          : f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
            for (int c = sub; c < D; c += lpr) dst[c] = src ? src[c] : 0.f;
        }
    }
    // the normalising groups run the shuffles; the others feed them a dummy (valid) row and discard
    const bool norm = live && src && normalise;
    const float *vs = norm ? src : mode_emb;
    if (norm) row_norm_store_sub(vs, dst, D, sub, lpr, vec);
    else {
        float dummy = 0.f;
        for (int off = lpr >> 1; off > 0; off >>= 1) dummy += __shfl_xor(dummy, off, 64);   // keep lanes converged
        (void)dummy;
    }
}

// ------------------------------------------------------------------------------------ layer levels
template <int MODE>
__global__ __launch_bounds__(256) void step_layer_fwd_kernel(const StepDev *__restrict__ sd, LayerPtrs lp, int p,
                                                             const TileRef *__restrict__ tiles,
                                                             const float *__restrict__ Hin,
                                                             float *__restrict__ Hout) {
    __shared__ __attribute__((aligned(16))) float smem[GT_SMEM_FLOATS];
    const TileRef tr = tiles[blockIdx.x];
    const BatchDev &b = sd->b[tr.batch];
    const int D = sd->D;
    const int ct = (D + GT_BN - 1) / GT_BN;
    const int n = tr.node, rem = tr.rem;
    const int li = layer_index(p, b.L, sd->num_layers);
    const TmplArgs tp = b.tp;
    tmpl_fwd_tile<MODE>(tp, b.B, Hin + b.row_off * D, pick_layer(lp.basis, li), pick_layer(lp.root, li),
                        pick_layer(lp.bias, li), D, D, p < b.L - 1,
                       Hout + b.row_off * D, n, (long long)(rem / ct) * GT_BM, (rem % ct) * GT_BN, smem);
}

template <int MODE>
__global__ __launch_bounds__(256) void step_layer_bwd_x_kernel(const StepDev *__restrict__ sd, LayerPtrs lp, int p,
                                                               const TileRef *__restrict__ tiles,
                                                               const float *__restrict__ Gout,
                                                               const float *__restrict__ Hin,
                                                               float *__restrict__ Gin, int add_in) {
    __shared__ __attribute__((aligned(16))) float smem[GT_SMEM_FLOATS];
    const TileRef tr = tiles[blockIdx.x];
    const BatchDev &b = sd->b[tr.batch];
    const int D = sd->D;
    const int ct = (D + GT_BN - 1) / GT_BN;
    const int m = tr.node, rem = tr.rem;
    const int li = layer_index(p, b.L, sd->num_layers);
    const TmplArgs tp = b.tp;
    // Gout is already a pre-activation gradient (masked by whoever wrote it); the gradient written
    // here belongs to H[p], which for p >= 1 is the ReLU output of pass p-1 -> mask it on the way out
    tmpl_bwd_x_tile<MODE>(tp, b.B, Gout + b.row_off * D, (const float *)nullptr, pick_layer(lp.basis, li),
                          pick_layer(lp.root, li), D, D, 0,
                         Gin + b.row_off * D, m, (long long)(rem / ct) * GT_BM, (rem % ct) * GT_BN, smem,
                         p >= 1 ? Hin + b.row_off * D : (const float *)nullptr, b.live[p + 1], add_in && p >= 1);
}

// ------------------------------------------------------------------------------------ score / loss
__device__ __forceinline__ float readout_value(int readout, const float *__restrict__ h, int N, int A, int D,
                                               int c, int *arg) {
    if (readout == MPQE_READOUT_TM) return h[(long long)A * D + c];
    if (readout == MPQE_READOUT_SUM) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += h[(long long)n * D + c];
        return s;
    }
    float best = h[c];
    int a = 0;
    for (int n = 1; n < N; ++n) {
        const float v = h[(long long)n * D + c];
        if (v > best) {
            best = v;
            a = n;
        }
    }
    *arg = a;
    return best;
}

#define STEP_MAX_COLS_PER_LANE 8     // D <= 512 on the fused path

// wave per graph, NJ = ceil(D / 64) columns per lane (compile-time: keeps the per-lane arrays in
// registers). BWD = false: scores and hinge terms. BWD = true: gradient rows of gH[L_b] and the
// positive / negative target-table gradients (through the L2 normalisation).
template <bool BWD, int NJ>
__global__ __launch_bounds__(256) void step_score_kernel(
    const StepDev *__restrict__ sd, const float *__restrict__ H, long long level_stride,
    const float *__restrict__ tpos, const float *__restrict__ tneg, float margin, float eps,
    float *__restrict__ s_pos, float *__restrict__ s_neg, float *__restrict__ terms,
    float *__restrict__ GH, TablePtrs tabs, const long long *__restrict__ node_map, long long map_len,
    const long long *__restrict__ targets, const long long *__restrict__ negs, long long g0, long long ng,
    const float *__restrict__ Q, float *__restrict__ GQ, const float *__restrict__ RY, float *__restrict__ RGY,
    int ro_op) {
    // Q != NULL (MPQE_READOUT_CALLER): the query embedding of graph gi is row gi of Q, its gradient goes to row gi of GQ.
    // RY != NULL (the learned readouts, step_readout.h): the embedding is the add / max / mean (ro_op: MPQE_SCATTER_*) over the
    // graph's rows of RY -- its N node rows, or its N - 1 pair rows (TARGETMLP) -- and the rows' gradients go to RGY.
    const long long gl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (gl >= ng) return;
    const long long gi = g0 + gl;          // graphs [g0, g0 + ng): one stream lane of the step
    int bi = 0;
    for (int i = 1; i < sd->nb; ++i)
        if (sd->b[i].g_off <= gi) bi = i;
    const BatchDev &b = sd->b[bi];
    const int D = sd->D, N = b.tp.N, A = b.A;
    const long long row0 = b.row_off + (gi - b.g_off) * N;
    const float *h = H + (long long)b.L * level_stride + row0 * D;
    const bool ro_pairs = RY && sd->readout == MPQE_READOUT_TARGETMLP;
    const int ro_cnt = ro_pairs ? N - 1 : N;
    const long long ro_r0 = ro_pairs ? (b.row_off - b.g_off) + (gi - b.g_off) * (N - 1) : row0;
    if (RY) h = RY + ro_r0 * D;
    const float *tp_ = tpos + gi * D, *tn_ = tneg + gi * D;
    float q[NJ];
    int arg[NJ];
    float dp = 0.f, dn = 0.f, qq = 0.f, pp = 0.f, nn = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        q[j] = 0.f;
        arg[j] = 0;
        if (c < D) {
            if (RY) {
                q[j] = readout_value(ro_op == MPQE_SCATTER_MAX ? MPQE_READOUT_MAX : MPQE_READOUT_SUM, h, ro_cnt, 0, D, c, &arg[j]);
                if (ro_op == MPQE_SCATTER_MEAN) q[j] /= (float)ro_cnt;
            } else q[j] = Q ? Q[gi * D + c] : readout_value(sd->readout, h, N, A, D, c, &arg[j]);
            const float a = tp_[c], bb = tn_[c];
            dp += q[j] * a;
            dn += q[j] * bb;
            qq += q[j] * q[j];
            pp += a * a;
            nn += bb * bb;
        }
    }
    dp = wave_sum(dp);
    dn = wave_sum(dn);
    qq = wave_sum(qq);
    pp = wave_sum(pp);
    nn = wave_sum(nn);
    const float rq = sqrtf(qq), rp = sqrtf(pp), rn = sqrtf(nn);
    const float nq = fmaxf(rq, eps), np_ = fmaxf(rp, eps), nn_ = fmaxf(rn, eps);
    const float sp = dp / (nq * np_), sn = dn / (nq * nn_);
    const float v = margin - (sp - sn);
    if (lane == 0) {        // the backward instance also emits the scores: no separate forward launch then
        s_pos[gi] = sp;
        s_neg[gi] = sn;
        terms[gi] = v > 0.f ? v : 0.f;
    }
    if (!BWD) return;
    // d loss / d sp = -w/B on active terms, d/d sn = +w/B   (loss = sum_b w_b mean_b hinge)
    const float act = v >= 0.f ? b.weight / (float)b.B : 0.f;
    const float gsp = -act, gsn = act;
    const float inv_p = 1.f / (nq * np_), inv_n = 1.f / (nq * nn_);
    const float kq = rq > eps ? (gsp * sp + gsn * sn) / (nq * nq) : 0.f;
    const float ktp = rp > eps ? sp / (np_ * np_) : 0.f;
    const float ktn = rn > eps ? sn / (nn_ * nn_) : 0.f;
    // target rows: y = v/|v| (unit norm), dv = (g - y (y.g)) / |v|; |v| from the table row
    const int tab = b.target_tab;
    const long long prow = table_row(node_map, map_len, targets[gi], tabs.rows[tab], nullptr);
    const long long nrow = table_row(node_map, map_len, negs[gi], tabs.rows[tab], nullptr);
    float gyp[NJ], gyn[NJ];
    float yg_p = 0.f, yg_n = 0.f, ssp = 0.f, ssn = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        gyp[j] = gyn[j] = 0.f;
        if (c < D) {
            const float a = tp_[c], bb = tn_[c];
            gyp[j] = gsp * (q[j] * inv_p - ktp * a);
            gyn[j] = gsn * (q[j] * inv_n - ktn * bb);
            yg_p += a * gyp[j];
            yg_n += bb * gyn[j];
            if (prow >= 0) {
                const float t = tabs.table[tab][prow * D + c];
                ssp += t * t;
            }
            if (nrow >= 0) {
                const float t = tabs.table[tab][nrow * D + c];
                ssn += t * t;
            }
            const float gq = gsp * tp_[c] * inv_p + gsn * tn_[c] * inv_n - kq * q[j];
            float *gh = GH + (long long)b.L * level_stride + row0 * D + c;
            if (Q) GQ[gi * D + c] = gq;
            if (RY) {
                float *gy = RGY + ro_r0 * D + c;
                for (int n = 0; n < ro_cnt; ++n)
                    gy[(long long)n * D] = ro_op == MPQE_SCATTER_ADD ? gq
                                           : (ro_op == MPQE_SCATTER_MEAN ? gq / (float)ro_cnt : (arg[j] == n ? gq : 0.f));
            }
            for (int n = 0; n < N && !Q && !RY; ++n) {
                float gv;
                if (sd->readout == MPQE_READOUT_SUM) gv = gq;
                else if (sd->readout == MPQE_READOUT_TM) gv = n == A ? gq : 0.f;
                else gv = arg[j] == n ? gq : 0.f;
                gh[(long long)n * D] = gv;
            }
        }
    }
    yg_p = wave_sum(yg_p);
    yg_n = wave_sum(yg_n);
    ssp = wave_sum(ssp);
    ssn = wave_sum(ssn);
    const float ivp = 1.f / sqrtf(ssp), ivn = 1.f / sqrtf(ssn);
    float *gt = tabs.grad[tab];
    if (gt) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = lane + 64 * j;
            if (c < D) {
                if (prow >= 0) atomicAdd(gt + prow * D + c, (gyp[j] - tp_[c] * yg_p) * ivp);
                if (nrow >= 0) atomicAdd(gt + nrow * D + c, (gyn[j] - tn_[c] * yg_n) * ivn);
            }
        }
    }
}

// loss[0] = sum_b w_b * mean_b(terms), loss[1 + b] = mean_b(terms): one workgroup of 16 waves, wave b
// sums batch b (lane-strided, then a butterfly), thread 0 adds the batches in order -> fixed order
// nwaves waves of the calling workgroup take the batches round-robin (fixed order per batch, and the
// total is added in batch order by thread 0): reproducible.
__device__ __forceinline__ void loss_block(const StepDev *__restrict__ sd, const float *__restrict__ terms,
                                           float *__restrict__ loss, float *mean /*LDS, MAX_BATCHES floats*/,
                                           int nwaves) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int bi = w; bi < sd->nb; bi += nwaves) {
        const BatchDev &b = sd->b[bi];
        float s = 0.f;
        for (int i = lane; i < b.B; i += 64) s += terms[b.g_off + i];
        s = wave_sum(s);
        if (lane == 0) {
            mean[bi] = s / (float)b.B;
            loss[1 + bi] = mean[bi];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.f;
        for (int bi = 0; bi < sd->nb; ++bi) total += sd->b[bi].weight * mean[bi];
        loss[0] = total;
    }
}

__global__ __launch_bounds__(1024) void step_loss_kernel(const StepDev *__restrict__ sd,
                                                         const float *__restrict__ terms,
                                                         float *__restrict__ loss, LossMeta lm,
                                                         const float *__restrict__ bterms, unsigned *epoch_f,
                                                         int bump_b = 0, unsigned *notify = nullptr, unsigned notify_value = 0,
                                                         const int32_t *err = nullptr) {
    __shared__ float mean[MPQE_STEP_MAX_BATCHES];
    // (mpqe_step_extra_t.notify: this is the forward-only call's last launch -- the launches that read the ids have run)
    if (notify && threadIdx.x == 0) {
        notify[1] = err ? (unsigned)*err : 0u;
#ifndef MPQE_EMU
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");            // (system scope: the flags word is out before the number)
#endif
        notify[0] = notify_value;
    }
    // (forward-only step: this is its last launch -- the next step's forward granules get a new tag, step_uniform.h; and
    // when its chain launch made transposed copies -- a learned readout's forward reads them -- their count a new target)
    if (epoch_f && threadIdx.x == 0) {
        *epoch_f = *epoch_f + 1u;
        if (bump_b) *(epoch_f + 16) = *(epoch_f + 16) + 1u;
    }
    if (lm.chain) loss_block_chain(lm, bterms, loss, mean, 16);
    else loss_block(sd, terms, loss, mean, 16);
}

#include "step_tail.h"
#include "step_plan.h"

// diagnostics: phase time stamps of the chain kernel's workgroups (tools/chain_timeline.py)
static long long *g_tail_stamps = nullptr;
static size_t g_tail_stamp_blocks = 0;
extern "C" void mpqe_debug_tail_stamps(void *device_buffer, size_t num_blocks) {
    g_tail_stamps = reinterpret_cast<long long *>(device_buffer);
    g_tail_stamp_blocks = num_blocks;
}
static long long *g_chain_stamps = nullptr;
static size_t g_chain_stamp_blocks = 0;
extern "C" void mpqe_debug_chain_stamps(void *device_buffer, size_t num_blocks) {
    g_chain_stamps = reinterpret_cast<long long *>(device_buffer);
    g_chain_stamp_blocks = num_blocks;
}

// Chain kernels (step_chain.h): D = 64 / 128 / 256 with 16-byte aligned weights, every batch within the number of
// passes the kernel's LDS tables cover. Everything else takes the one-launch-per-level form.
static bool want_chain(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb);
// plan for (P, B, lanes): the recent one if it matches, else a fresh one (which becomes the recent one)
static std::shared_ptr<CachedPlan> plan_for(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb,
                                            const mpqe_step_lanes_t *lanes, int *status) {
    *status = MPQE_OK;
    if (!P || !B || nb < 1 || nb > MPQE_STEP_MAX_BATCHES) {
        *status = MPQE_ERR_INVALID_ARG;
        return nullptr;
    }
    const bool ask_chain = want_chain(P, B, nb);
    PlanKey key;
    make_key(P, B, nb, lanes, &key);
    key.chain = ask_chain ? 1 : 0;
    {
        std::lock_guard<std::mutex> lock(g_plan_mu);
        if (g_recent && memcmp(&g_recent->key, &key, sizeof(key)) == 0) return g_recent;
    }
    std::shared_ptr<CachedPlan> fresh = std::make_shared<CachedPlan>();
    fresh->key = key;
    *status = plan_auto(P, B, nb, lanes, ask_chain, &fresh->hp);
    if (*status) return nullptr;
    std::lock_guard<std::mutex> lock(g_plan_mu);
    g_recent = fresh;
    return fresh;
}

// The launch plan is a pure function of the descriptors; it is kept on the host next to the device
// table it describes (same key: the caller's desc buffer), so a steady-state call costs one lookup.
// upload_desc NULL: look up only (the plan of a step that has run from `desc` with these descriptors, or none). Otherwise a
// plan that is not there is made, and *upload_desc is raised where this call has to write the table again.
static int plan_lookup(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb, const mpqe_step_lanes_t *lanes,
                       void *desc, int *upload_desc, std::shared_ptr<const CachedPlan> *out) {
    const bool ask_chain = want_chain(P, B, nb);
    PlanKey key;
    make_key(P, B, nb, lanes, &key);
    key.chain = ask_chain ? 1 : 0;
    std::lock_guard<std::mutex> lock(g_plan_mu);
    auto it = g_plans.find(desc);
    if (it != g_plans.end() && memcmp(&it->second->key, &key, sizeof(key)) == 0) {
        *out = it->second;
        return MPQE_OK;
    }
    if (!upload_desc) return MPQE_ERR_INVALID_ARG;
    if (it != g_plans.end() && !*upload_desc) {
        // desc holds another step's table -- unless only the diagnostics switches changed since it was planned: then the
        // same step is planned again and its table uploaded again by this call
        PlanKey old = it->second->key;
        old.dbg_gen = key.dbg_gen;
        if (memcmp(&old, &key, sizeof(key)) != 0) return MPQE_ERR_INVALID_ARG;
        *upload_desc = 1;
    }
    // (the size queries of this packed step have just built it)
    std::shared_ptr<CachedPlan> plan = g_recent && memcmp(&g_recent->key, &key, sizeof(key)) == 0 ? g_recent : nullptr;
    if (!plan) {
        plan = std::make_shared<CachedPlan>();
        plan->key = key;
        const int st = plan_auto(P, B, nb, lanes, ask_chain, &plan->hp);
        if (st) return st;
    }
    if (g_plans.size() >= 1024) g_plans.clear();      // plans in use stay alive through their shared_ptr
    g_plans[desc] = plan;
    *out = plan;
    return MPQE_OK;
}

static bool want_chain(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb) {
    if (!P || !B || nb < 1 || nb > MPQE_STEP_MAX_BATCHES) return false;
    bool use_chain = !(P->flags & MPQE_STEP_NO_CHAIN) && (P->dim == 64 || P->dim == 128 || P->dim == 256) &&
                     (P->readout < MPQE_READOUT_CALLER || P->readout >= MPQE_READOUT_MLP);
    // (the caller's readout needs the node states in HBM: level form. The learned readouts: two more levels of the chain,
    // while the ReLU bits of their hidden rows have a level to live in and two layer slots are free for their parameters)
    if (!use_chain) return false;
    if (P->readout >= MPQE_READOUT_MLP) {
        if (P->readout == MPQE_READOUT_CONCAT) {        // (one input block per layer)
            for (int i = 0; i < nb; ++i)
                if (B[i].num_passes != P->num_layers) return false;
        }
        if (P->num_layers + 2 > MPQE_STEP_MAX_LAYERS || !P->readout_w0 || !P->readout_w2) return false;
        if (!ptr_vec_ok(P->readout_w0, P->dim) || !ptr_vec_ok(P->readout_w2, P->dim)) return false;
        if ((P->readout_b0 && (uintptr_t)P->readout_b0 % 16 != 0) || (P->readout_b2 && (uintptr_t)P->readout_b2 % 16 != 0)) return false;
        for (int i = 0; i < nb; ++i)
            if (B[i].num_passes + 1 > CH_MASK_LEVELS) return false;
    }
    long long graphs = 0;
    for (int i = 0; i < nb; ++i) graphs += B[i].batch_size;
    use_chain = graphs <= CHAIN_MAX_GRAPHS && P->num_layers > 0 && P->num_layers <= MPQE_STEP_MAX_LAYERS;
    // (5 passes x (3 edges + 4 nodes) x 2 directions = 70 ops <= CH_MAX_OPS; a batch with more than CH_MAX_CV forward
    // node updates is turned away by the planner: plan_auto)
    for (int i = 0; i < nb; ++i) use_chain = use_chain && B[i].num_passes <= CH_MASK_LEVELS + 1;
    for (int l = 0; use_chain && l < P->num_layers; ++l)
        use_chain = P->basis[l] && P->root[l] && ptr_vec_ok(P->basis[l], P->dim) && ptr_vec_ok(P->root[l], P->dim) &&
                    (!P->bias[l] || (uintptr_t)P->bias[l] % 16 == 0);
    for (int m = 0; use_chain && m < P->num_modes && m < MPQE_STEP_MAX_MODES; ++m)
        use_chain = P->tables[m] && (uintptr_t)P->tables[m] % 16 == 0;
    return use_chain && P->mode_emb && (uintptr_t)P->mode_emb % 16 == 0;
}

extern "C" size_t mpqe_step_workspace_bytes(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb,
                                            const mpqe_step_lanes_t *lanes) {
    int st;
    const std::shared_ptr<CachedPlan> cp = plan_for(P, B, nb, lanes, &st);
    return cp ? cp->hp.total : 0;
}
extern "C" size_t mpqe_step_desc_bytes(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb,
                                       const mpqe_step_lanes_t *lanes) {
    // exact: the level form's lanes have their own per-level tile tables, so the table's size depends on the split
    int st;
    const std::shared_ptr<CachedPlan> cp = plan_for(P, B, nb, lanes, &st);
    return cp ? cp->hp.desc_total : 0;
}

extern "C" int mpqe_step_states_layout(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb,
                                       const mpqe_step_lanes_t *lanes, int64_t *states_offset, int64_t *grads_offset,
                                       int64_t *level_stride, int64_t *row_offset, int64_t *queries_offset,
                                       int64_t *query_grads_offset) {
    int st;
    const std::shared_ptr<CachedPlan> cp = plan_for(P, B, nb, lanes, &st);
    if (!cp) return st ? st : MPQE_ERR_INVALID_ARG;
    const HostPlan &hp = cp->hp;
    if (hp.chain || P->readout != MPQE_READOUT_CALLER) return MPQE_ERR_UNSUPPORTED;        // (the chain form keeps the node states in LDS)
    if (states_offset) *states_offset = (int64_t)hp.o_H;
    if (grads_offset) *grads_offset = (int64_t)hp.o_GH;
    if (level_stride) *level_stride = (int64_t)hp.level_stride;
    if (queries_offset) *queries_offset = (int64_t)hp.o_Q;
    if (query_grads_offset) *query_grads_offset = (int64_t)hp.o_GQ;
    for (int i = 0; row_offset && i <= nb; ++i) row_offset[i] = i < nb ? (int64_t)hp.sd.b[i].row_off : (int64_t)hp.sd.rows_total;
    return MPQE_OK;
}

// ---- touch plan (step_touch.h)
static int touch_dims(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb, long long *M, int *row_bits,
                      int *key_bits) {
    if (!P || !B || nb < 1 || nb > MPQE_STEP_MAX_BATCHES || P->num_modes <= 0 || P->num_modes > MPQE_STEP_MAX_MODES)
        return MPQE_ERR_INVALID_ARG;
    *M = touch_entries(B, nb);
    if (*M <= 0 || *M >= (1ll << 31)) return MPQE_ERR_INVALID_ARG;
    long long rows = 1;
    for (int m = 0; m < P->num_modes; ++m) rows = std::max(rows, (long long)P->table_rows[m]);
    *row_bits = touch_bits(rows);
    *key_bits = *row_bits + 5;          // table index (<= 16) above the row; an invalid entry has every bit set
    return MPQE_OK;
}
extern "C" size_t mpqe_step_touch_bytes(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb) {
    long long M;
    int rb, kb;
    if (touch_dims(P, B, nb, &M, &rb, &kb) != MPQE_OK) return 0;
    return touch_layout(M, kb).total;
}
extern "C" size_t mpqe_step_touch_workspace_bytes(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb) {
    long long M;
    int rb, kb;
    if (touch_dims(P, B, nb, &M, &rb, &kb) != MPQE_OK) return 0;
    return touch_layout(M, kb).w_total;
}
extern "C" int mpqe_step_touch_build(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb,
                                     const int64_t *anchor_ids, const int64_t *targets, const int64_t *negs,
                                     void *touch, size_t touch_bytes, void *workspace, size_t workspace_bytes,
                                     void *stream) {
    long long M;
    int rb, kb;
    int st = touch_dims(P, B, nb, &M, &rb, &kb);
    if (st) return st;
    if (!anchor_ids || !targets || !negs || !touch || !workspace || !P->node_map) return MPQE_ERR_INVALID_ARG;
    const TouchLayout L = touch_layout(M, kb);
    if (touch_bytes < L.total || workspace_bytes < L.w_total) return MPQE_ERR_WORKSPACE;
    if ((uintptr_t)touch % 256 != 0 || (uintptr_t)workspace % 256 != 0) return MPQE_ERR_INVALID_ARG;
    hipStream_t s = as_stream(stream);
    TouchMeta tm;
    memset(&tm, 0, sizeof(tm));
    tm.nb = nb;
    tm.row_bits = rb;
    long long anchors = 0, graphs = 0;
    for (int i = 0; i < nb; ++i) {
        const TemplateDesc &t = kTemplates[B[i].query_type];
        tm.B[i] = B[i].batch_size;
        tm.A[i] = t.A;
        tm.anchor_off[i] = anchors;
        tm.g_off[i] = graphs;
        for (int a = 0; a < 3; ++a) {
            tm.anchor_tab[i][a] = a < t.A ? B[i].anchor_mode[a] : 0;
            if (a < t.A && (B[i].anchor_mode[a] < 0 || B[i].anchor_mode[a] >= P->num_modes)) return MPQE_ERR_INVALID_ARG;
        }
        if (B[i].target_mode < 0 || B[i].target_mode >= P->num_modes) return MPQE_ERR_INVALID_ARG;
        tm.target_tab[i] = B[i].target_mode;
        anchors += (long long)B[i].batch_size * t.A;
        graphs += B[i].batch_size;
    }
    tm.anchor_off[nb] = anchors;
    tm.g_off[nb] = graphs;
    for (int m = 0; m < P->num_modes; ++m) tm.table_rows[m] = P->table_rows[m];
    char *tb = reinterpret_cast<char *>(touch), *wb = reinterpret_cast<char *>(workspace);
    TouchHeader th;
    memset(&th, 0, sizeof(th));
    th.M = M;
    th.row_bits = rb;
    th.key_bits = kb;
    static_assert(sizeof(TouchMeta) <= 2048, "touch_layout reserves 2 KB for the batch table");
    if (M <= TSORT_MAX_ENTRIES && kb <= 31 && !dbg_on("TOUCH_MULTI_LAUNCH") && !(P->flags & MPQE_STEP_TOUCH_LIBRARY_SORT)) {
        // the whole plan in one launch (step_touch.h: tsort_block) behind the clear of its barrier counter and the
        // upload of the batch table
        const int nblk = tsort_blocks(M);
        const size_t Mp = (size_t)nblk * TSORT_THREADS * tsort_rounds(M);
        TSortArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.ka = reinterpret_cast<unsigned *>(wb + L.w_keys);
        sa.kb = sa.ka + Mp;                                   // (the 8-byte key array, halved)
        sa.va = reinterpret_cast<unsigned *>(wb + L.w_vals);
        sa.vb = reinterpret_cast<unsigned *>(wb + L.w_svals);
        sa.hist = reinterpret_cast<unsigned *>(wb + L.w_hist);
        sa.counter = sa.hist + 4 * 256 * 256;
        TouchMeta *tmd = reinterpret_cast<TouchMeta *>(sa.counter + 64);
        sa.tm = tmd;
        (void)hipMemsetAsync(sa.counter, 0, sizeof(unsigned), s);
        upload(s, reinterpret_cast<char *>(tmd), &tm, sizeof(tm));
        sa.anchor_ids = reinterpret_cast<const long long *>(anchor_ids);
        sa.targets = reinterpret_cast<const long long *>(targets);
        sa.negs = reinterpret_cast<const long long *>(negs);
        sa.node_map = reinterpret_cast<const long long *>(P->node_map);
        sa.map_len = (long long)P->node_map_len;
        sa.keys_out = reinterpret_cast<tkey_t *>(tb + L.keys);
        sa.perm = reinterpret_cast<int *>(tb + L.perm);
        sa.erow = reinterpret_cast<int *>(tb + L.erow);
        sa.th_out = reinterpret_cast<TouchHeader *>(tb);
        sa.M = (int)M;
        sa.key_bits = kb;
        sa.row_bits = rb;
        sa.nblk = nblk;
        sa.rounds = tsort_rounds(M);
        hipLaunchKernelGGL(touch_sort_kernel, dim3((unsigned)nblk), dim3(TSORT_THREADS), 0, s, sa);
        return mpqe_launch_status();
    }
    // (the header rides along as an argument of the keys kernel; the sort leaves perm = the entries in sorted order)
    tkey_t *keys = reinterpret_cast<tkey_t *>(wb + L.w_keys);
    int *vals = reinterpret_cast<int *>(wb + L.w_vals);
    hipLaunchKernelGGL(touch_keys_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, tm,
                       reinterpret_cast<const long long *>(anchor_ids), reinterpret_cast<const long long *>(targets),
                       reinterpret_cast<const long long *>(negs), reinterpret_cast<const long long *>(P->node_map),
                       (long long)P->node_map_len, keys, vals, reinterpret_cast<int *>(tb + L.erow), M, th,
                       reinterpret_cast<TouchHeader *>(tb));
    // stable: entries of one destination row keep their entry order, so the per-row sums have ONE order (radix_sort.h: the
    // library's own multi-launch sort -- nothing in it depends on how many workgroups are resident at once)
    if (radix_sort_pairs_own<tkey_t>(wb + L.w_tmp, (const tkey_t *)keys, reinterpret_cast<tkey_t *>(tb + L.keys), (const int *)vals,
                                     reinterpret_cast<int *>(tb + L.perm), (long long)M, kb, s))
        return MPQE_ERR_LAUNCH;
    return mpqe_launch_status();
}

// ---- row-sparse Adam over the touched table rows (include/mpqe_amd.h: mpqe_adam_rows_step)
struct RowAdamPtrs {
    float *p[MPQE_STEP_MAX_MODES], *m[MPQE_STEP_MAX_MODES], *v[MPQE_STEP_MAX_MODES];
    const float *g[MPQE_STEP_MAX_MODES];
};
__global__ __launch_bounds__(256) void adam_rows_kernel(const TouchHeader *__restrict__ th, const tkey_t *__restrict__ keys,
                                                        int D, RowAdamPtrs rp, float omb1, float omb2, float eps,
                                                        float neg_step_size, const int32_t *__restrict__ guard,
                                                        long long *__restrict__ applied) {
    // (mpqe_adam_rows_step_guarded: the step's error word, read once per workgroup before any store -- csrc/optim.hip)
    if (guard && *guard != 0) return;
    if (applied && blockIdx.x == 0 && threadIdx.x == 0) *applied += 1;
    // one group of D / 4 lanes per sorted position; the first position of a run of equal keys owns the row
    const int lpr = D / 4, per = 256 / lpr;
    const long long k = (long long)blockIdx.x * per + threadIdx.x / lpr;
    const int c = (threadIdx.x % lpr) * 4;
    if (k >= th->M) return;
    const tkey_t key = keys[k];
    if (key == TOUCH_INVALID || (k > 0 && keys[k - 1] == key)) return;
    const int tab = (int)(key >> th->row_bits);
    const long long off = (long long)(key & ((1ull << th->row_bits) - 1ull)) * D + c;
    float *p = rp.p[0], *m = rp.m[0], *v = rp.v[0];
    const float *g = rp.g[0];
#pragma unroll
    for (int t = 1; t < MPQE_STEP_MAX_MODES; ++t)
        if (t == tab) {
            p = rp.p[t];
            m = rp.m[t];
            v = rp.v[t];
            g = rp.g[t];
        }
    if (!p || !g || !m || !v) return;
    const f32x4 gg = gload4(g + off);
    f32x4 pp = *reinterpret_cast<f32x4 *>(p + off), mm = *reinterpret_cast<f32x4 *>(m + off);
    f32x4 vv = *reinterpret_cast<f32x4 *>(v + off);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        // torch.optim.SparseAdam, operation for operation (no contraction into fused multiply-adds: the same roundings)
        const float m_upd = __fmul_rn(__fsub_rn(gg[e], mm[e]), omb1);
        const float v_upd = __fmul_rn(__fsub_rn(__fmul_rn(gg[e], gg[e]), vv[e]), omb2);
        const float numer = __fadd_rn(m_upd, mm[e]);
        const float v_new = __fadd_rn(v_upd, vv[e]);
        const float denom = __fadd_rn(sqrtf(v_new), eps);
        mm[e] = __fadd_rn(mm[e], m_upd);
        vv[e] = v_new;
        pp[e] = __fadd_rn(pp[e], __fmul_rn(neg_step_size, __fdiv_rn(numer, denom)));
    }
    *reinterpret_cast<f32x4 *>(p + off) = pp;
    *reinterpret_cast<f32x4 *>(m + off) = mm;
    *reinterpret_cast<f32x4 *>(v + off) = vv;
}

extern "C" int64_t mpqe_step_touch_entries(const mpqe_step_batch_t *B, int nb) {
    if (!B || nb < 1 || nb > MPQE_STEP_MAX_BATCHES) return -1;
    return touch_entries(B, nb);
}

// ---- a plan from (table, row) keys that are given, not looked up (the data-parallel row exchange: every rank's touched
// rows, all-gathered): keys sorted (stable), perm[k] = index of sorted position k in the input order
extern "C" size_t mpqe_rows_plan_bytes(int64_t n) { return n > 0 ? touch_layout(n, 0).total : 0; }
extern "C" size_t mpqe_rows_plan_workspace_bytes(int64_t n, int key_bits) {
    return n > 0 && key_bits > 0 && key_bits <= 64 ? touch_layout(n, key_bits).w_total : 0;
}
__global__ __launch_bounds__(256) void iota_kernel(int *__restrict__ v, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = (int)i;
}
extern "C" int mpqe_rows_plan_build(const uint64_t *keys, int64_t n, int row_bits, int key_bits, void *plan,
                                    size_t plan_bytes, void *workspace, size_t workspace_bytes, void *stream) {
    if (!keys || !plan || !workspace || n <= 0 || n >= (1ll << 31) || row_bits <= 0 || key_bits <= row_bits || key_bits > 64)
        return MPQE_ERR_INVALID_ARG;
    const TouchLayout L = touch_layout(n, key_bits);
    if (plan_bytes < L.total || workspace_bytes < L.w_total) return MPQE_ERR_WORKSPACE;
    if ((uintptr_t)plan % 256 != 0 || (uintptr_t)workspace % 256 != 0) return MPQE_ERR_INVALID_ARG;
    hipStream_t s = as_stream(stream);
    char *tb = reinterpret_cast<char *>(plan), *wb = reinterpret_cast<char *>(workspace);
    TouchHeader th;
    memset(&th, 0, sizeof(th));
    th.M = n;
    th.row_bits = row_bits;
    th.key_bits = key_bits;
    upload(s, tb, &th, sizeof(th));
    int *vals = reinterpret_cast<int *>(wb + L.w_vals);
    hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, vals, (long long)n);
    if (radix_sort_pairs_own<tkey_t>(wb + L.w_tmp, reinterpret_cast<const tkey_t *>(keys), reinterpret_cast<tkey_t *>(tb + L.keys),
                                     (const int *)vals, reinterpret_cast<int *>(tb + L.perm), (long long)n, key_bits, s))
        return MPQE_ERR_LAUNCH;
    return mpqe_launch_status();
}
// table_grads[t][row] (= or +=) the sum of rows[perm[k]] over the plan's run of key (t, row), in sorted (= input) order
__global__ __launch_bounds__(256) void rows_sum_kernel(const char *__restrict__ plan, size_t o_keys, size_t o_perm,
                                                       const float *__restrict__ rows, int D, TablePtrs tabs, int store) {
    const TouchHeader *th = reinterpret_cast<const TouchHeader *>(plan);
    table_sum_block(th->M, th->row_bits, reinterpret_cast<const tkey_t *>(plan + o_keys),
                    reinterpret_cast<const int *>(plan + o_perm), rows, D, tabs, store, (long long)blockIdx.x);
}
extern "C" int mpqe_table_rows_sum(const void *plan, int64_t n, const float *rows, int64_t dim, float *const *table_grads,
                                   int num_modes, int store, void *stream) {
    if (!plan || !rows || !table_grads || n <= 0 || num_modes <= 0 || num_modes > MPQE_STEP_MAX_MODES)
        return MPQE_ERR_INVALID_ARG;
    if (dim <= 0 || dim % 4 != 0 || dim > 1024 || 256 % (dim / 4) != 0 || (uintptr_t)rows % 16 != 0) return MPQE_ERR_UNSUPPORTED;
    TablePtrs tabs;
    memset(&tabs, 0, sizeof(tabs));
    for (int m = 0; m < num_modes; ++m) {
        tabs.grad[m] = table_grads[m];
        if ((uintptr_t)table_grads[m] % 16 != 0) return MPQE_ERR_INVALID_ARG;
    }
    const TouchLayout L = touch_layout(n, 0);
    const long long per = 256 / (dim / 4);
    hipLaunchKernelGGL(rows_sum_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const char *>(plan), L.keys, L.perm, rows, (int)dim, tabs, store);
    return mpqe_launch_status();
}

// The entity-table rows of a step's reduction again (include/mpqe_amd.h): a step whose own touch plan could not be built
// (MPQE_FLAG_TOUCH_RETRY) left every entry's gradient row in its workspace; `touch` is a plan built afterwards.
__global__ __launch_bounds__(256) void step_table_rows_kernel(const char *__restrict__ touch, size_t o_keys, size_t o_perm,
                                                              long long M, int row_bits, const float *__restrict__ DG, int D,
                                                              TablePtrs tabs, int store) {
    table_sum_block(M, row_bits, reinterpret_cast<const tkey_t *>(touch + o_keys), reinterpret_cast<const int *>(touch + o_perm),
                    DG, D, tabs, store, (long long)blockIdx.x, &reinterpret_cast<const TouchHeader *>(touch)->pad[0]);
}
extern "C" int mpqe_step_table_rows(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb, const mpqe_step_grads_t *G,
                                    const void *desc, void *workspace, size_t workspace_bytes, const void *touch, void *stream) {
    if (!P || !B || !G || !desc || !workspace || !touch || nb < 1 || nb > MPQE_STEP_MAX_BATCHES) return MPQE_ERR_INVALID_ARG;
    if ((uintptr_t)touch % 256 != 0 || (uintptr_t)workspace % 256 != 0) return MPQE_ERR_INVALID_ARG;
    std::shared_ptr<const CachedPlan> cached;
    // (refused: not the descriptor buffer of a step that has run with these descriptors)
    if (plan_lookup(P, B, nb, nullptr, const_cast<void *>(desc), nullptr, &cached)) return MPQE_ERR_INVALID_ARG;
    const HostPlan &hp = cached->hp;
    if (!hp.chain || hp.touch_M <= 0) return MPQE_ERR_UNSUPPORTED;
    if (workspace_bytes < hp.total) return MPQE_ERR_WORKSPACE;
    const int D = P->dim;
    if (D % 4 != 0 || 256 % (D / 4) != 0) return MPQE_ERR_UNSUPPORTED;
    long long trows = 1;
    TablePtrs tabs;
    memset(&tabs, 0, sizeof(tabs));
    for (int m = 0; m < P->num_modes; ++m) {
        trows = std::max(trows, (long long)P->table_rows[m]);
        tabs.grad[m] = G->tables[m];
        tabs.rows[m] = P->table_rows[m];
        if (G->tables[m] && (uintptr_t)G->tables[m] % 16 != 0) return MPQE_ERR_INVALID_ARG;
    }
    const TouchLayout TL = touch_layout(hp.touch_M, 0);
    const long long per = 256 / (D / 4);
    const int store = ((P->flags & MPQE_STEP_SPARSE_TABLES) || (P->flags & MPQE_STEP_ZERO_GRADS)) ? 1 : 0;
    hipLaunchKernelGGL(step_table_rows_kernel, dim3((unsigned)((hp.touch_M + per - 1) / per)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const char *>(touch), TL.keys, TL.perm, (long long)hp.touch_M, touch_bits(trows),
                       reinterpret_cast<const float *>(reinterpret_cast<const char *>(workspace) + hp.o_DG), D, tabs, store);
    return mpqe_launch_status();
}

static int adam_rows_launch(const void *touch, int64_t num_entries, float *const *params, const float *const *grads,
                            float *const *exp_avg, float *const *exp_avg_sq, int num_modes, int64_t dim, double lr,
                            double beta1, double beta2, double eps, int64_t step, const int32_t *guard, int64_t *applied,
                            void *stream) {
    if (!touch || num_entries <= 0 || !params || !grads || !exp_avg || !exp_avg_sq || step < 1) return MPQE_ERR_INVALID_ARG;
    if (num_modes <= 0 || num_modes > MPQE_STEP_MAX_MODES || dim <= 0 || dim % 4 != 0 || dim > 1024 || 256 % (dim / 4) != 0)
        return MPQE_ERR_UNSUPPORTED;
    if (!(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1.)) return MPQE_ERR_INVALID_ARG;
    const long long M = num_entries;
    RowAdamPtrs rp;
    memset(&rp, 0, sizeof(rp));
    for (int m = 0; m < num_modes; ++m) {
        rp.p[m] = params[m];
        rp.g[m] = grads[m];
        rp.m[m] = exp_avg[m];
        rp.v[m] = exp_avg_sq[m];
        if (((uintptr_t)rp.p[m] | (uintptr_t)rp.g[m] | (uintptr_t)rp.m[m] | (uintptr_t)rp.v[m]) % 16 != 0)
            return MPQE_ERR_INVALID_ARG;
    }
    // torch.optim.SparseAdam: step_size = lr * sqrt(1 - b2^t) / (1 - b1^t) in double (python floats), 1 - beta too
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const float neg_step = (float)(-(lr * sqrt(bc2) / bc1));
    const TouchLayout L = touch_layout(M, 0);
    const char *tb = reinterpret_cast<const char *>(touch);
    const long long per = 256 / (dim / 4);
    hipLaunchKernelGGL(adam_rows_kernel, dim3((unsigned)((M + per - 1) / per)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const TouchHeader *>(tb), reinterpret_cast<const tkey_t *>(tb + L.keys), (int)dim, rp,
                       (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, neg_step, guard,
                       reinterpret_cast<long long *>(applied));
    return mpqe_launch_status();
}

extern "C" int mpqe_adam_rows_step(const void *touch, int64_t num_entries, float *const *params,
                                   const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                                   int num_modes, int64_t dim, double lr, double beta1, double beta2, double eps,
                                   int64_t step, void *stream) {
    return adam_rows_launch(touch, num_entries, params, grads, exp_avg, exp_avg_sq, num_modes, dim, lr, beta1, beta2, eps,
                            step, nullptr, nullptr, stream);
}

extern "C" int mpqe_adam_rows_step_guarded(const void *touch, int64_t num_entries, float *const *params,
                                           const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                                           int num_modes, int64_t dim, double lr, double beta1, double beta2, double eps,
                                           int64_t step, const int32_t *guard, int64_t *applied, void *stream) {
    if (!guard) return MPQE_ERR_INVALID_ARG;
    return adam_rows_launch(touch, num_entries, params, grads, exp_avg, exp_avg_sq, num_modes, dim, lr, beta1, beta2, eps,
                            step, guard, applied, stream);
}

// sum_i ||p_i||_2 of up to four parameter tensors and its backward (the regulariser of margin_loss, reference
// model.py:486-490, for the module path; the fused step calls the same kernel inside its own call)
extern "C" int mpqe_l2_norms(const float *const *params, const int64_t *sizes, int count, const float *grad_out, float *out,
                             float *const *grads, void *stream) {
    if (!params || !sizes || count < 1 || count > 4 || (!out && !grads)) return MPQE_ERR_INVALID_ARG;
    RoRegArgs rr;
    memset(&rr, 0, sizeof(rr));
    for (int i = 0; i < count; ++i) {
        if (!params[i] || sizes[i] <= 0) return MPQE_ERR_INVALID_ARG;
        rr.p[i] = params[i];
        rr.n[i] = sizes[i];
        rr.g[i] = grads ? grads[i] : nullptr;
    }
    rr.coef = 1.f;
    rr.loss = out;                 // (+= : the caller zero-fills it)
    rr.gscale = grad_out;
    hipLaunchKernelGGL(step_ro_reg_kernel, dim3(1), dim3(1024), 0, as_stream(stream), rr);
    return mpqe_launch_status();
}

static int D_ok_for_readout(int D) { return D % 4 == 0; }      // (16-byte rows in step_readout.h)
// input width of the learned readout's first Linear layer (reference model.py:497-553: targetmlp [target | node], concat one
// block per layer)
static int readout_kin(const mpqe_step_params_t *P) {
    return P->readout == MPQE_READOUT_TARGETMLP ? 2 * P->dim : (P->readout == MPQE_READOUT_CONCAT ? P->num_layers * P->dim : P->dim);
}

// batch weights of a call with extras: sd->b[i].weight = host weight x *device scalar (one workgroup, in front of the step's
// launches on its stream; wdev[i] NULL: the host weight alone -- which is also how a later call without extras restores them)
struct WeightPatch {
    const float *wdev[MPQE_STEP_MAX_BATCHES];
    float whost[MPQE_STEP_MAX_BATCHES];
    int nb;
};
__global__ __launch_bounds__(64) void step_weights_kernel(StepDev *sd, WeightPatch wp) {
    const int i = threadIdx.x;
    if (i < wp.nb) sd->b[i].weight = wp.wdev[i] ? wp.whost[i] * *wp.wdev[i] : wp.whost[i];
}

extern "C" int mpqe_step_readout_norms(const mpqe_step_params_t *P, float *out, void *stream) {
    if (!P || !out || P->readout < MPQE_READOUT_MLP) return MPQE_ERR_INVALID_ARG;
    if (!P->readout_w0 || !P->readout_b0 || !P->readout_w2 || !P->readout_b2 || P->dim <= 0) return MPQE_ERR_INVALID_ARG;
    const int D = P->dim, kin = D_ok_for_readout(D) ? readout_kin(P) : 0;
    if (kin <= 0) return MPQE_ERR_UNSUPPORTED;
    RoRegArgs rr;
    memset(&rr, 0, sizeof(rr));
    rr.p[0] = P->readout_w0; rr.p[1] = P->readout_b0; rr.p[2] = P->readout_w2; rr.p[3] = P->readout_b2;
    rr.n[0] = (long long)D * kin; rr.n[1] = D; rr.n[2] = (long long)D * D; rr.n[3] = D;
    rr.coef = 1.f;                       // (out = fma(1, sum of the norms, 0): the sum itself)
    rr.loss = out;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(out, 0, sizeof(float), s) != hipSuccess) return MPQE_ERR_LAUNCH;
    hipLaunchKernelGGL(step_ro_reg_kernel, dim3(1), dim3(1024), 0, s, rr);
    return mpqe_launch_status();
}

extern "C" int mpqe_step_forward_backward(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb,
                                          const int64_t *anchor_ids, const int64_t *targets, const int64_t *negs,
                                          float margin, const mpqe_step_grads_t *G, int backward,
                                          float *loss, float *scores_pos, float *scores_neg, void *desc,
                                          size_t desc_bytes, int upload_desc, void *workspace,
                                          size_t workspace_bytes, int32_t *err, const mpqe_step_lanes_t *lanes,
                                          void *const *events, int num_events, void *touch, void *stream) {
    return mpqe_step_forward_backward_ex(P, B, nb, anchor_ids, targets, negs, margin, G, backward, loss, scores_pos, scores_neg,
                                         desc, desc_bytes, upload_desc, workspace, workspace_bytes, err, lanes, events, num_events,
                                         touch, stream, nullptr);
}

// the step's host driver: plan lookup, argument checks, the two launch forms, mpqe_step_forward_backward_ex
#include "step_drive.h"
