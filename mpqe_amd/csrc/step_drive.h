// Part of csrc/step.hip (one translation unit; included there behind the step's other entry points): the host driver of
// the fused step, mpqe_step_forward_backward_ex. step_ex() looks the launch plan up (plan_lookup), checks every argument
// (step_check) before anything is queued, resolves the call into one context (StepCtx) and hands it to one of two launch
// forms, each a straight sequence of launches:
//   run_level_form   one launch per level and lane, node states in HBM: dimensions other than 64 / 128 / 256,
//                    MPQE_STEP_NO_CHAIN, the three-call phases round a caller's readout, the learned readouts off the chain
//   run_chain_form   one chain launch, then nothing (merged tail) or the weight-gradient launch, then the reduction
// The launches both forms share (weight gradients, reduction, loss, readout regulariser, lane fork / join) and the choice of
// a kernel's template instance are plain functions over the context.
#pragma once
// the arguments of mpqe_step_forward_backward_ex (include/mpqe_amd.h) as one value
struct StepCall {
    const mpqe_step_params_t *P;
    const mpqe_step_batch_t *B;
    int nb;
    const int64_t *anchor_ids, *targets, *negs;
    float margin;
    const mpqe_step_grads_t *G;
    int phase;                  // (the API's `backward`: 0 / 1, or MPQE_STEP_PHASE_* round a caller's readout)
    float *loss, *scores_pos, *scores_neg;
    void *desc;
    size_t desc_bytes;
    int upload_desc;
    void *workspace;
    size_t workspace_bytes;
    int32_t *err;
    const mpqe_step_lanes_t *lanes;
    void *const *events;
    int num_events;
    void *touch, *stream;
    const mpqe_step_extra_t *extra;
};

// One call of the step after its plan is known: what both launch forms read. Built once per call (step_flags, step_resolve,
// step_launch_args); afterwards only the event cursor, zmats_in_chain and ra.nmat change.
struct StepCtx : StepCall {     // (upload_desc: possibly raised by the plan lookup)
    std::shared_ptr<const CachedPlan> cached;
    const HostPlan *hp;
    // phase = 2 .. 5: the step in three calls around a readout the CALLER computes (include/mpqe_amd.h: MPQE_STEP_PHASE_*,
    // MPQE_READOUT_CALLER; level form, every node state live)
    bool phase_fwd, phase_bwd, phase_score;
    bool chain, backward, learned, merged, use_touch, build_touch, sparse_tables, dev_weights;
    bool zero_fill;             // this call fills the gradients with zeros (step in several calls: the first one fills)
    int add_states, touch_row_bits;
    int D, NL;
    hipStream_t s, ls[MPQE_STEP_MAX_LANES];
    char *wb, *db;
    int ev;                     // event cursor (mark)
    unsigned *notify, notify_value;
    LayerPtrs lp; GradPtrs gp;
    TablePtrs tabs; LossMeta lm;
    int vec, vec_tab; bool fast;      // 16-byte rows of the weights / the tables and mode vectors; and whole tiles
    int vec_grad;                     // 16-byte rows of every gradient buffer the reduction launch reads and writes
    const StepDev *sd;
    unsigned *epoch_f, *epoch_b;
    float *H, *GH, *VT, *WT, *slabs, *parts, *terms, *tpos, *tneg, *spos, *sneg;
    const float *bterms;
    const long long *ids, *tg, *ng, *nm;
    long long row0[MPQE_STEP_MAX_LANES + 1], gr0[MPQE_STEP_MAX_LANES + 1];
    // arguments of the launches both forms share (step_launch_args)
    TailArgs ta; UArgs ub; ReduceArgs ra;
    unsigned r_gx, r_trows;     // the reduction launch's row width; its entity-table gradient rows
    bool use_runs, zmats_in_chain;     // (zmats_in_chain: the chain launch has zero-filled the untouched relation matrices)
};

// typed pointer into the workspace / the descriptor table
template <class T>
static T *at(char *base, size_t offset) { return reinterpret_cast<T *>(base + offset); }
// what the call asks for, from its arguments and its plan (no checks: step_check comes next)
static void step_flags(StepCtx &c) {
    const HostPlan &hp = *c.hp;
    c.chain = hp.chain;
    c.phase_fwd = c.phase == MPQE_STEP_PHASE_STATES;
    c.phase_bwd = c.phase == MPQE_STEP_PHASE_FROM_STATES;
    c.phase_score = c.phase == MPQE_STEP_PHASE_SCORES || c.phase == MPQE_STEP_PHASE_SCORES_ONLY;
    c.learned = c.P->readout >= MPQE_READOUT_MLP;       // (step_readout.h: the readout's two Linear layers are the library's too)
    // (the caller's readout read every level: its gradients of the intermediate levels are in the workspace already)
    c.add_states = ((c.phase_bwd && (c.P->flags & MPQE_STEP_ADD_STATE_GRADS)) || c.P->readout == MPQE_READOUT_CONCAT) ? 1 : 0;
    // (PHASE_SCORES_ONLY: scores and loss from the caller's embeddings, no gradients)
    c.backward = c.phase != 0 && c.phase != MPQE_STEP_PHASE_SCORES_ONLY;
    // touch plan given: the chain form stores per-entry table-gradient rows and sums them per destination (no atomics)
    c.use_touch = c.touch != nullptr && c.chain && c.backward;
    // ... BUILD_TOUCH: `touch` is an OUTPUT -- the step builds the plan of the ids it is called with inside its chain launch
    // (the level form has no use for a plan and leaves the buffer alone, as it ignores a plan built at pack time)
    c.build_touch = c.use_touch && (c.P->flags & MPQE_STEP_BUILD_TOUCH) != 0;
    c.sparse_tables = (c.P->flags & MPQE_STEP_SPARSE_TABLES) != 0;
    c.touch_row_bits = 1;         // (= the header of the caller's plan: mpqe_step_touch_build derives it the same way)
    if (c.use_touch) {
        long long trows = 1;
        for (int m = 0; m < c.P->num_modes; ++m) trows = std::max(trows, (long long)c.P->table_rows[m]);
        c.touch_row_bits = touch_bits(trows);
    }
    c.D = c.P->dim;
    c.NL = hp.nlanes;
    // merged launch: tiles + post-pass ride in the chain launch (include/mpqe_amd.h: MPQE_STEP_MERGE_TAIL)
    // Measured (AIFB mix, D = 128, B per batch 32 / 64 / 128 / 256 / 384 / 512 / 8192): merged 48.9 / 50.3 / 52.6 / 56.8 /
    // 61.3 / 68.4 / 569 us per step against 59.8 / 59.4 / 62.0 / 62.9 / 64.8 / 65.2 / 550 -- it wins while the chain
    // workgroups leave a free slot on (almost) every CU, and loses once the tiles have to share CUs with running chain
    // workgroups and queue behind them. Hence: merged up to 9/8 x CUs chain workgroups unless a flag says otherwise.
    c.merged = c.chain && c.backward && c.NL == 1 && !(c.P->flags & MPQE_STEP_SPLIT_TAIL) &&
               ((c.P->flags & MPQE_STEP_MERGE_TAIL) || hp.blk_off[c.nb] <= STEP_CUS + STEP_CUS / 8);
    c.zero_fill = c.backward && !c.phase_bwd && !c.phase_score && (c.P->flags & MPQE_STEP_ZERO_GRADS);
    for (int i = 0; c.extra && i < c.nb; ++i) c.dev_weights = c.dev_weights || c.extra->batch_weight[i] != nullptr;
    c.notify = c.extra ? reinterpret_cast<unsigned *>(c.extra->notify) : nullptr;
    c.notify_value = c.extra ? c.extra->notify_value : 0u;
}
// every gradient buffer but the entity tables' on a 16-byte boundary (NULL: not wanted). readout: a learned readout's too
// (the chain form's virtual layers; off the chain they are the dense layer's, which looks at its own pointers)
static bool grads_vec_ok(const StepCall &c, bool readout) {
    const mpqe_step_grads_t &G = *c.G;
    uintptr_t bits = (uintptr_t)G.mode_emb;
    for (int l = 0; l < c.P->num_layers; ++l) bits |= (uintptr_t)G.basis[l] | (uintptr_t)G.root[l] | (uintptr_t)G.bias[l];
    if (readout && c.P->readout >= MPQE_READOUT_MLP)
        bits |= (uintptr_t)G.readout_w0 | (uintptr_t)G.readout_b0 | (uintptr_t)G.readout_w2 | (uintptr_t)G.readout_b2;
    return bits % 16 == 0;
}
// every argument check of the step, in front of its first queued operation
static int step_check(const StepCtx &c) {
    const HostPlan &hp = *c.hp;
    if (c.phase < 0 || c.phase > MPQE_STEP_PHASE_SCORES_ONLY) return MPQE_ERR_INVALID_ARG;
    if ((c.phase >= 2) != (c.P->readout == MPQE_READOUT_CALLER)) return MPQE_ERR_INVALID_ARG;
    if ((c.phase >= 2 || c.learned) && ((c.chain && !hp.ro_chain) || hp.nlanes > 1)) return MPQE_ERR_UNSUPPORTED;
    if (c.learned) {
        if (!c.P->readout_w0 || !c.P->readout_b0 || !c.P->readout_w2 || !c.P->readout_b2) return MPQE_ERR_INVALID_ARG;
        if (c.P->readout_scatter < MPQE_SCATTER_ADD || c.P->readout_scatter > MPQE_SCATTER_MEAN) return MPQE_ERR_INVALID_ARG;
        if (D_ok_for_readout(c.P->dim) == 0) return MPQE_ERR_UNSUPPORTED;
        if (c.backward && c.G && (!c.G->readout_w0 || !c.G->readout_b0 || !c.G->readout_w2 || !c.G->readout_b2)) return MPQE_ERR_INVALID_ARG;
        if (c.P->readout == MPQE_READOUT_CONCAT)
            for (int i = 0; i < c.nb; ++i)
                if (hp.sd.b[i].L != c.P->num_layers) return MPQE_ERR_INVALID_ARG;     // (model.py:441-446: one input block per layer)
    }
    if (c.build_touch && (hp.ts_blocks <= 0 || (c.P->flags & MPQE_STEP_EIGHT_WAVES) || hp.nlanes > 1))
        return MPQE_ERR_UNSUPPORTED;        // (a step beyond TSORT_MAX_ENTRIES ids: build the plan at pack time)
    if (c.sparse_tables && c.backward && !c.use_touch) return MPQE_ERR_INVALID_ARG;      // (needs the touch plan and the chain form)
    // (the chain form's kernels move whole 16-byte pieces of the gradient buffers; the level form takes any float pointer:
    // step_resolve picks its scalar forms)
    if (c.chain && c.backward && c.G && !grads_vec_ok(c, true)) return MPQE_ERR_INVALID_ARG;
    if (c.use_touch) {
        if ((uintptr_t)c.touch % 256 != 0) return MPQE_ERR_INVALID_ARG;
        for (int m = 0; m < c.P->num_modes; ++m)
            if (c.G->tables[m] && (uintptr_t)c.G->tables[m] % 16 != 0) return MPQE_ERR_INVALID_ARG;
    }
    for (int l = 1; l < hp.nlanes; ++l)           // handles are per call, not part of the cached plan
        if (!c.lanes->fork_event || !c.lanes->aux_stream[l] || !c.lanes->join_event[l]) return MPQE_ERR_INVALID_ARG;
    if (!c.anchor_ids || !c.targets || !c.negs || !c.loss || !c.workspace) return MPQE_ERR_INVALID_ARG;
    if (c.desc_bytes < hp.desc_total) return MPQE_ERR_WORKSPACE;
    if ((uintptr_t)c.desc % 256 != 0) return MPQE_ERR_INVALID_ARG;
    if (c.backward && !c.G) return MPQE_ERR_INVALID_ARG;
    if (c.workspace_bytes < hp.total) return MPQE_ERR_WORKSPACE;
    if ((uintptr_t)c.workspace % 256 != 0) return MPQE_ERR_INVALID_ARG;
    if (!c.P->node_map || !c.P->mode_emb) return MPQE_ERR_INVALID_ARG;
    for (int l = 0; l < c.P->num_layers; ++l)
        if (!c.P->basis[l] || !c.P->root[l]) return MPQE_ERR_INVALID_ARG;
    for (int m = 0; m < c.P->num_modes; ++m)
        if (!c.P->tables[m]) return MPQE_ERR_INVALID_ARG;
    if (c.extra && c.extra->query_out && !c.chain) return MPQE_ERR_UNSUPPORTED;       // (the chain workgroups' score phase writes it)
    return MPQE_OK;
}
// streams, parameter / gradient pointers, workspace and descriptor pointers of a checked call
static void step_resolve(StepCtx &c) {
    const HostPlan &hp = *c.hp;
    const int D = c.D, nb = c.nb;
    c.s = as_stream(c.stream);
    c.wb = reinterpret_cast<char *>(c.workspace);
    c.db = reinterpret_cast<char *>(c.desc);
    c.ls[0] = c.s;
    for (int l = 1; l < c.NL; ++l) c.ls[l] = as_stream(c.lanes->aux_stream[l]);
    memset(&c.lp, 0, sizeof(c.lp));
    memset(&c.gp, 0, sizeof(c.gp));
    memset(&c.tabs, 0, sizeof(c.tabs));
    c.vec = D % 4 == 0;
    for (int l = 0; l < c.P->num_layers; ++l) {
        c.lp.basis[l] = c.P->basis[l]; c.lp.root[l] = c.P->root[l]; c.lp.bias[l] = c.P->bias[l];
        c.vec = c.vec && ptr_vec_ok(c.P->basis[l], D) && ptr_vec_ok(c.P->root[l], D);
        if (c.backward) {
            c.gp.basis[l] = c.G->basis[l]; c.gp.root[l] = c.G->root[l]; c.gp.bias[l] = c.G->bias[l];
        }
    }
    if (hp.ro_chain) {       // the readout's Linear layers: virtual layers of the chain form (HostPlan.ro_chain)
        c.lp.root[hp.ro_layer] = c.P->readout_w0; c.lp.bias[hp.ro_layer] = c.P->readout_b0;
        c.lp.root[hp.ro_layer + 1] = c.P->readout_w2; c.lp.bias[hp.ro_layer + 1] = c.P->readout_b2;
        if (c.backward) {
            c.gp.root[hp.ro_layer] = c.G->readout_w0; c.gp.bias[hp.ro_layer] = c.G->readout_b0;
            c.gp.root[hp.ro_layer + 1] = c.G->readout_w2; c.gp.bias[hp.ro_layer + 1] = c.G->readout_b2;
        }
    }
    // (the assemble kernel reads the table rows and the mode vectors with the same loads)
    c.vec_tab = D % 4 == 0 && (uintptr_t)c.P->mode_emb % 16 == 0;
    c.vec_grad = D % 4 == 0 && (!c.backward || grads_vec_ok(c, c.chain));
    for (int m = 0; m < c.P->num_modes; ++m) {
        c.vec_tab = c.vec_tab && (uintptr_t)c.P->tables[m] % 16 == 0;
        c.tabs.table[m] = c.P->tables[m]; c.tabs.rows[m] = c.P->table_rows[m];
        c.tabs.grad[m] = c.backward ? c.G->tables[m] : nullptr;
    }
    if (c.backward) c.gp.mode_emb = c.G->mode_emb;
    c.fast = c.vec && D % GT_BN == 0;     // D is both K (multiple of 32) and the tile width (64)
    c.sd = at<const StepDev>(c.db, hp.o_sd);
    c.epoch_f = at<unsigned>(c.db, hp.o_epoch); c.epoch_b = c.epoch_f + 16;
    c.H = at<float>(c.wb, hp.o_H); c.GH = at<float>(c.wb, hp.o_GH);
    c.VT = at<float>(c.wb, hp.o_VT); c.WT = at<float>(c.wb, hp.o_WT);
    c.tpos = at<float>(c.wb, hp.o_tpos); c.tneg = at<float>(c.wb, hp.o_tneg);
    c.spos = c.scores_pos ? c.scores_pos : at<float>(c.wb, hp.o_spos);
    c.sneg = c.scores_neg ? c.scores_neg : at<float>(c.wb, hp.o_sneg);
    c.terms = at<float>(c.wb, hp.o_terms); c.bterms = at<const float>(c.wb, hp.o_bterms);
    c.slabs = at<float>(c.wb, hp.o_slabs); c.parts = at<float>(c.wb, hp.o_parts);
    c.ids = reinterpret_cast<const long long *>(c.anchor_ids); c.nm = reinterpret_cast<const long long *>(c.P->node_map);
    c.tg = reinterpret_cast<const long long *>(c.targets); c.ng = reinterpret_cast<const long long *>(c.negs);
    // Stream lanes: lane l runs the whole dependent chain (assemble -> levels -> score -> levels back)
    // of ITS batches on its own stream, so the ~8 us a short launch costs regardless of its size
    // overlaps with the other lanes' work; the lanes meet again before the weight gradients.
    for (int l = 0; l <= c.NL; ++l) {
        const int b = hp.lane_begin[l];
        c.row0[l] = b < nb ? hp.sd.b[b].row_off : hp.sd.rows_total;
        c.gr0[l] = b < nb ? hp.sd.b[b].g_off : hp.sd.graphs_total;
    }
    memset(&c.lm, 0, sizeof(c.lm));
    c.lm.nb = nb; c.lm.chain = c.chain ? 1 : 0;
    for (int i = 0; i < nb; ++i) {
        c.lm.B[i] = hp.sd.b[i].B; c.lm.weight[i] = hp.sd.b[i].weight; c.lm.blk_off[i] = hp.blk_off[i];
    }
    c.lm.blk_off[nb] = hp.blk_off[nb];
}
// the call's first queued operations: the descriptor table where it is asked for, the batch weights where they are not the plan's
static void queue_descriptors(const StepCtx &c) {
    const HostPlan &hp = *c.hp;
    if (c.upload_desc) {
        // the descriptor table: ONE copy of the host image the plan keeps (the plan outlives the call: the cache holds
        // it); then the hand-off state of this packed step: epochs 0, every granule tagged 0 (a live tag is >= 1)
        (void)hipMemcpyAsync(c.db, hp.image.data(), hp.image.size(), hipMemcpyHostToDevice, c.s);
        (void)hipMemsetAsync(c.db + hp.o_epoch, 0, hp.desc_total - hp.o_epoch, c.s);
    }
    if (c.dev_weights || (c.cached->weights_patched && !c.upload_desc)) {
        WeightPatch wp;
        memset(&wp, 0, sizeof(wp));
        wp.nb = c.nb;
        for (int i = 0; i < c.nb; ++i) {
            wp.whost[i] = hp.sd.b[i].weight;
            wp.wdev[i] = c.dev_weights ? c.extra->batch_weight[i] : nullptr;
        }
        hipLaunchKernelGGL(step_weights_kernel, dim3(1), dim3(64), 0, c.s, const_cast<StepDev *>(c.sd), wp);
    }
    c.cached->weights_patched = c.dev_weights;
}
// batch-uniform node states: what the forward pre-pass (chain launch) and the backward post-pass share
static UArgs uniform_args(const StepCtx &c) {
    UArgs ua;
    memset(&ua, 0, sizeof(ua));
    ua.chunks = c.D / 64;
    ua.VT = c.VT; ua.gran = at<u64>(c.db, c.hp->o_gran); ua.mode_emb = c.P->mode_emb;
    ua.num_modes = (long long)c.P->num_modes; ua.parts = c.parts; ua.err = c.err;
    return ua;
}
// arguments of the weight-gradient launch (ta, ub) and of the step's reduction, a launch of its own (ra)
static void step_launch_args(StepCtx &c) {
    const HostPlan &hp = *c.hp;
    const int D = c.D;
    char *db = c.db, *wb = c.wb;
    TailArgs &ta = c.ta;          // (what is not named here stays 0: the context is value-initialised)
    ta.wsrc = at<const WSource>(db, hp.o_wsrc); ta.nwsrc = (int)hp.wsrc.size();
    ta.wblock = at<const WBlock>(db, hp.o_wblock); ta.wblocks = hp.wblocks_total;
    ta.vsrc = at<const VSource>(db, hp.o_vsrc); ta.nvsrc = (int)hp.vsrc.size();
    ta.vblock = at<const int>(db, hp.o_vblock); ta.vblocks = hp.vblocks_total;
    ta.anchor_off = at<const int>(db, hp.o_anchor); ta.anchor_ids = c.ids;
    ta.nb = c.nb; ta.D = D; ta.tile_n = hp.tile_n;
    ta.node_map = c.nm; ta.map_len = (long long)c.P->node_map_len;
    ta.slabs = c.slabs; ta.parts = c.parts;
    ta.zmats = at<const ZMat>(db, hp.o_zmats);
    ta.zper = (int)(((long long)D * D + ZMAT_FLOATS_PER_BLOCK - 1) / ZMAT_FLOATS_PER_BLOCK);
    c.ub = uniform_args(c);
    c.ub.ops = at<const UOp>(db, hp.o_uopb); c.ub.nops = (int)hp.uops_b.size(); c.ub.epoch = c.epoch_b;
    ReduceArgs &ra = c.ra;
    memset(&ra, 0, sizeof(ra));
    ra.nmat = -1;
    c.r_gx = (unsigned)(((long long)D * D + 255) / 256);
    c.r_trows = 0;         // entity-table gradient rows: 256 / (D / 4) sorted positions per workgroup
    if (c.use_touch && !(STEP_DBG & 1)) {
        const long long per = 256 / (D / 4), tblk = (hp.touch_M + per - 1) / per;
        c.r_trows = (unsigned)((tblk + c.r_gx - 1) / c.r_gx);
    }
    ra.groups = at<const RGroup>(db, hp.o_groups); ra.ngroups = (int)hp.groups.size();
    ra.D = D; ra.vec = c.vec_grad; ra.zeroed = (c.P->flags & MPQE_STEP_ZERO_GRADS) ? 1 : 0;
    ra.gp = c.gp; ra.tabs = c.tabs; ra.lm = c.lm; ra.sd = c.sd;
    ra.slabs = c.slabs; ra.partial = c.parts; ra.VT = c.VT; ra.rank1 = at<const Rank1>(db, hp.o_rank1);
    ra.terms = c.terms; ra.bterms = c.bterms; ra.loss = c.loss;
    ra.epoch_b = c.chain ? c.epoch_b : nullptr;
    ra.touch = c.use_touch ? reinterpret_cast<const char *>(c.touch) : nullptr;
    ra.touch_keys = touch_layout(hp.touch_M, 0).keys; ra.touch_perm = touch_layout(hp.touch_M, 0).perm;
    ra.touch_M = (long long)hp.touch_M; ra.touch_row_bits = c.touch_row_bits;
    ra.DG = at<const float>(wb, hp.o_DG);
    ra.table_store = ((c.sparse_tables || (c.P->flags & MPQE_STEP_ZERO_GRADS)) ? 1 : 0) | (c.merged ? 2 : 0);
    ra.err = c.err; ra.notify = c.notify; ra.notify_value = c.notify_value;
    // (the loss and the entity-table rows of the split tail as a light launch of their own beside the weight-gradient launch
    // -- enqueued behind it with hipExtAnyOrderLaunch, i.e. without the queue's barrier bit -- was tried: the flag is not
    // honoured on gfx9 boards (hip_ext.h says so): the launch ran in order and the step took 4.4 us longer)
    // The table workgroups of the reduction launch take the plan's RUN STARTS, compacted by one workgroup of the weight-gradient
    // launch (touch_runs_block), instead of every sorted position: a step's distinct rows are at most the tables' rows -- the
    // launch is sized for that bound (AIFB step: 326 workgroups instead of 2 752). mpqe_debug_option NO_RUNS = 1: as before.
    c.use_runs = c.use_touch && !c.merged && c.NL == 1 && D % 4 == 0 && 256 % (D / 4) == 0 && !(STEP_DBG & 1) && !dbg_on("NO_RUNS");
    if (c.use_runs) {
        long long total_rows = 0;
        for (int m = 0; m < c.P->num_modes; ++m) total_rows += c.P->table_rows[m];
        const long long rmax = std::min<long long>(hp.touch_M, total_rows), per = 256 / (D / 4);
        c.r_trows = (unsigned)(((rmax + per - 1) / per + c.r_gx - 1) / c.r_gx);
        ra.runs = at<const int>(wb, hp.o_runs);
    }
}
// optional timing: event pair k brackets one launch, recorded on the stream of that launch (see mpqe_amd.h for the
// order). The cursor advances even when no event is left: the position in the array is the contract.
static void mark(StepCtx &c, hipStream_t on) {
    if (c.events && c.ev < c.num_events) (void)hipEventRecord(reinterpret_cast<hipEvent_t>(c.events[c.ev]), on);
    ++c.ev;
}
// fork: the lanes start after the descriptor uploads and the prologue
static void fork_lanes(const StepCtx &c) {
    if (c.NL <= 1) return;
    (void)hipEventRecord(reinterpret_cast<hipEvent_t>(c.lanes->fork_event), c.s);
    for (int l = 1; l < c.NL; ++l) (void)hipStreamWaitEvent(c.ls[l], reinterpret_cast<hipEvent_t>(c.lanes->fork_event), 0);
}
static void join_lanes(const StepCtx &c) {
    for (int l = 1; l < c.NL; ++l) {
        (void)hipEventRecord(reinterpret_cast<hipEvent_t>(c.lanes->join_event[l]), c.ls[l]);
        (void)hipStreamWaitEvent(c.s, reinterpret_cast<hipEvent_t>(c.lanes->join_event[l]), 0);
    }
}
// one more segment of a zero-fill list; `blocks`: the list's workgroups so far
static void zero_seg(ZeroSegs &zs, long long &blocks, float *ptr, long long n) {
    if (!ptr || n <= 0) return;
    for (int k = 0; k < zs.count; ++k)
        if (zs.p[k] == ptr) return;                  // shared layers repeat their buffers
    if (zs.count >= PREP_MAX_SEGS) return;
    zs.p[zs.count] = ptr;
    zs.n[zs.count] = n;
    zs.block0[zs.count] = blocks;
    blocks += (n + PREP_ZERO_FLOATS_PER_BLOCK - 1) / PREP_ZERO_FLOATS_PER_BLOCK;
    zs.count++;
}
static void grad_seg(const StepCtx &c, ZeroSegs &zs, long long &blocks, float *ptr, long long n) {
    // (merged launch: a root matrix that tiles / a rank-1 op of the SAME launch write whole is not zero-filled
    // -- the fill would race with its writers, who store instead of adding)
    for (size_t k = 0; c.merged && k < c.hp->whole_roots.size(); ++k)
        if (c.gp.root[c.hp->whole_roots[k]] == ptr) return;
    zero_seg(zs, blocks, ptr, n);
}
// the gradient buffers a call with zero_fill fills (`tables`: the entity tables' among them); returns the list's workgroups
static long long grad_zero_segs(const StepCtx &c, ZeroSegs &zs, bool tables) {
    const int D = c.D;
    long long blocks = 0;
    for (int l = 0; l < c.P->num_layers; ++l) {
        // (relation matrices: the written ones are stored by their writers, the untouched ones are zero-filled
        // by spare workgroups of the weight-gradient launch, off the critical path: ZMat)
        grad_seg(c, zs, blocks, c.G->root[l], (long long)D * D);
        grad_seg(c, zs, blocks, c.G->bias[l], D);
    }
    grad_seg(c, zs, blocks, c.G->mode_emb, (long long)c.P->num_modes * D);
    if (c.learned) {
        grad_seg(c, zs, blocks, c.G->readout_w0, (long long)D * c.hp->ro_kin);
        grad_seg(c, zs, blocks, c.G->readout_b0, D);
        grad_seg(c, zs, blocks, c.G->readout_w2, (long long)D * D);
        grad_seg(c, zs, blocks, c.G->readout_b2, D);
    }
    for (int m = 0; tables && m < c.P->num_modes; ++m) grad_seg(c, zs, blocks, c.G->tables[m], (long long)c.P->table_rows[m] * D);
    zs.block0[zs.count] = blocks;
    return blocks;
}
template <int MODE>
static void launch_tail_as(const StepCtx &c, dim3 grid, hipStream_t on, const TailArgs &tl) {
    hipLaunchKernelGGL(step_tail_kernel<MODE>, grid, dim3(256), 0, on, c.sd, tl, (const float *)c.H, (const float *)c.GH,
                       c.hp->level_stride, c.gp, (c.P->flags & MPQE_STEP_ZERO_GRADS) ? 1 : 0, c.lp, c.ub, c.ra);
}
// the weight-gradient launch over the whole block table on stream `on`
static void launch_grad_w(const StepCtx &c, hipStream_t on) {
    const HostPlan &hp = *c.hp;
    const int count = hp.wblocks_total;
    TailArgs tl = c.ta;
    if ((c.P->flags & MPQE_STEP_ZERO_GRADS) && !c.zmats_in_chain) tl.zblocks = (int)hp.zmats.size() * tl.zper;
    tl.ublocks = c.ub.nops * c.ub.chunks;
    int nblocks = tl.ublocks + count + tl.zblocks;
    // chain form: two of the eight XCDs for the post-pass' vector ops, six for the tiles (AIFB step, same box,
    // three runs each: 64.95 / 65.15 / 65.04 us against 65.70 / 65.60 / 65.47 with both kinds everywhere; one
    // or three XCDs: 65.8 / 66.0). mpqe_debug_option TAIL_UX overrides (0 = everywhere).
    const int uxv = mpqe_dbg_value("TAIL_UX", 2);
    // (only while the tiles are all resident at once on the other XCDs -- two per CU: with more of them the vector
    // ops' XCDs would stand idle for most of the launch. AIFB step with the MLP readout, 988 tiles: 64.3 -> 52.9 us)
    if (c.chain && tl.ublocks >= 4 && uxv > 0 && uxv < 8 &&
        (count <= (8 - uxv) * 2 * (STEP_CUS / STEP_XCDS) || mpqe_dbg_value("TAIL_UX", -1) > 0)) {
        tl.ux = uxv;
        const int ra = (tl.ublocks + tl.ux - 1) / tl.ux, rb = (count + tl.zblocks + (8 - tl.ux) - 1) / (8 - tl.ux);
        nblocks = 8 * (ra > rb ? ra : rb);
    }
    if (c.use_runs) {       // a few workgroups in front: the touch plan's run starts
        tl.runs_n = (int)((hp.touch_M + TRUNS_PER - 1) / TRUNS_PER);
        tl.runs_front = (tl.runs_n + 7) / 8 * 8;
        tl.runs_out = at<int>(c.wb, hp.o_runs);
        nblocks += tl.runs_front;
    }
    tl.stamps = g_tail_stamps && (size_t)nblocks <= g_tail_stamp_blocks ? g_tail_stamps : nullptr;
    if (nblocks <= 0) return;
    dim3 tgrid((unsigned)nblocks);
    // (chain form: ONE tile workgroup per CU -- the launch's LDS padded beyond half a CU's -- was measured on the 988-tile
    // step of the MLP readout: 71 - 75 us against 64; two per CU stay)
    if (c.chain) launch_tail_as<LD_T>(c, tgrid, on, tl);
    else if (c.fast && hp.whole_ksteps) launch_tail_as<LD_FAST>(c, tgrid, on, tl);
    else if (c.vec) launch_tail_as<LD_PRED>(c, tgrid, on, tl);
    else launch_tail_as<LD_SCALAR>(c, tgrid, on, tl);
}
// the step's reduction launch, bracketed by an event pair
static void launch_reduce(StepCtx &c) {
    const HostPlan &hp = *c.hp;
    // (matrix groups first in the table, vector groups behind them: then the vector groups share ONE row of the launch)
    int nmat = 0;
    const int ng = (int)hp.groups.size();
    while (nmat < ng && (hp.groups[nmat].kind <= 1 || hp.groups[nmat].kind >= 4)) ++nmat;
    bool packed = c.ra.vec && c.D % 4 == 0 && 256 % (c.D / 4) == 0 && !dbg_on("REDUCE_ROWS") && (ng - nmat) * VEC_SLICES + 1 <= (int)c.r_gx;
    for (int k = nmat; k < ng; ++k) packed = packed && (hp.groups[k].kind == 2 || hp.groups[k].kind == 3);
    c.ra.nmat = packed ? nmat : -1;
    dim3 grid(c.r_gx, (unsigned)(packed ? nmat + 1 : ng + 1) + c.r_trows);
    mark(c, c.s);
    hipLaunchKernelGGL(step_reduce_kernel, grid, dim3(256), 0, c.s, c.ra);
    mark(c, c.s);
}
// the loss of a forward-only step as a launch of its own (bump_b: the backward epoch advances too)
static void launch_loss(const StepCtx &c, int bump_b) {
    hipLaunchKernelGGL(step_loss_kernel, dim3(1), dim3(1024), 0, c.s, c.sd, (const float *)c.terms, c.loss, c.lm, c.bterms,
                       c.chain ? c.epoch_f : (unsigned *)nullptr, bump_b, c.notify, c.notify_value, (const int32_t *)c.err);
}
// the readout's regulariser (model.py:486-490), after the launch that writes loss[0]
static void ro_regulariser(const StepCtx &c, bool with_grads) {
    const HostPlan &hp = *c.hp;
    const int D = c.D, nb = c.nb;
    float wsum = 0.f;
    for (int i = 0; i < nb; ++i) wsum += hp.sd.b[i].weight;
    if (!(c.P->readout_weight_decay > 0.f)) return;
    RoRegArgs rr;
    memset(&rr, 0, sizeof(rr));
    rr.p[0] = c.P->readout_w0; rr.p[1] = c.P->readout_b0; rr.p[2] = c.P->readout_w2; rr.p[3] = c.P->readout_b2;
    rr.n[0] = (long long)D * hp.ro_kin; rr.n[1] = D; rr.n[2] = (long long)D * D; rr.n[3] = D;
    if (with_grads) { rr.g[0] = c.G->readout_w0; rr.g[1] = c.G->readout_b0; rr.g[2] = c.G->readout_w2; rr.g[3] = c.G->readout_b2; }
    rr.coef = c.P->readout_weight_decay * wsum; rr.loss = c.loss;
    if (c.dev_weights && with_grads) {        // (the gradients' coefficient: weight_decay x sum_i host_i x *device_i, formed on the device)
        rr.nw = nb; rr.wd = c.P->readout_weight_decay;
        for (int i = 0; i < nb; ++i) {
            rr.whost[i] = hp.sd.b[i].weight; rr.wdev[i] = c.extra->batch_weight[i];
        }
    }
    hipLaunchKernelGGL(step_ro_reg_kernel, dim3(1), dim3(1024), 0, c.s, rr);
}

// ------------------------------------------------------------------------------------ chain form
// the in-step touch plan (MPQE_STEP_BUILD_TOUCH): sort workgroups of the chain launch write the plan of this call's ids
static void touch_sort_args(const StepCtx &c, PrepArgs &pa) {
    const HostPlan &hp = *c.hp;
    const TouchLayout TL = touch_layout(hp.touch_M, 0);
    char *tb = reinterpret_cast<char *>(c.touch);
    const size_t Mp = (size_t)hp.ts_blocks * TSORT_THREADS * tsort_rounds(hp.touch_M);
    TSortArgs &ts = pa.ts;
    ts.tm = at<const TouchMeta>(c.db, hp.o_tmeta);
    ts.anchor_ids = c.ids; ts.targets = c.tg; ts.negs = c.ng;
    ts.node_map = c.nm; ts.map_len = (long long)c.P->node_map_len;
    ts.ka = at<unsigned>(c.wb, hp.o_tsort); ts.kb = ts.ka + Mp; ts.va = ts.kb + Mp; ts.vb = ts.va + Mp; ts.hist = ts.vb + Mp;
    ts.counter = c.epoch_f + 40;
    ts.keys_out = reinterpret_cast<tkey_t *>(tb + TL.keys); ts.perm = reinterpret_cast<int *>(tb + TL.perm);
    ts.erow = nullptr; ts.th_out = reinterpret_cast<TouchHeader *>(tb);
    ts.M = (int)hp.touch_M; ts.key_bits = hp.ts_key_bits; ts.row_bits = hp.ts_row_bits;
    ts.nblk = hp.ts_blocks; ts.rounds = tsort_rounds(hp.touch_M);
    ts.fail = dbg_on("TSORT_FAIL") ? 1 : 0; ts.stamps = nullptr;
    if (dbg_on("TSORT_TRAIL")) pa.strail = hp.ts_blocks;
    else {
        pa.sna = hp.sort_na; pa.sxrank = 0;
        for (int x = 0; x < STEP_XCDS; ++x) pa.sxrank |= (unsigned)(hp.sort_rank[x] + 1) << (4 * x);
        pa.sblocks = (hp.ts_blocks + pa.sna - 1) / pa.sna * 8;
    }
}
// prologue work: the forward pre-pass of the batch-uniform node states; backward: transposed weight copies for the
// backward chains, zero fill of the gradients (pa.zs, set by the caller) -- roles of the chain launch itself. Returns the
// transposed-copy workgroups of a full launch of this packed step.
static int chain_prologue(const StepCtx &c, PrepArgs &pa) {
    const HostPlan &hp = *c.hp;
    const int D = c.D, nb = c.nb, tpd = D / 64;
    pa.ua = uniform_args(c); pa.ua.ops = at<const UOp>(c.db, hp.o_uopf); pa.ua.nops = (int)hp.uops_f.size();
    pa.ua.epoch = c.epoch_f; pa.ublocks = pa.ua.nops * pa.ua.chunks;
    // (forward only: just the copies a learned readout's forward multiplies by -- the plan lists them last... not
    // sorted: all of them are made, the backward levels' are then unused)
    pa.tblocks = (c.backward || hp.ro_chain) ? (int)hp.wt_slots.size() * tpd * tpd : 0;
    const int wt_all = pa.tblocks;
    if (!c.backward && hp.ro_chain && !dbg_on("FWD_ALL_COPIES")) {
        // (the readout's forward multiplies by the TRANSPOSED blocks of its own two layers; the relation matrices'
        // copies and the plain column blocks belong to the backward programmes)
        int n = 0;
        bool fits = true;
        for (size_t k = 0; k < hp.wt_slots.size(); ++k)
            if (hp.wt_slots[k].mat < 0 && !hp.wt_slots[k].plain && hp.wt_slots[k].layer >= hp.ro_layer) {
                if (n < 8) pa.tsel[n] = (int)k;
                else fits = false;
                ++n;
            }
        if (fits && n > 0 && n < (int)hp.wt_slots.size()) {
            pa.tsel_n = n; pa.tblocks = n * tpd * tpd; pa.tskip = (unsigned)(wt_all - pa.tblocks);
        }
    }
    if (c.build_touch) touch_sort_args(c, pa);
    // The chain workgroups wait for vectors / matrices that the prologue workgroups produce, so the prologue
    // workgroups come first in the launch: a producer is never queued behind a consumer. (Every wait is bounded
    // all the same: a launch that could not make progress reports MPQE_FLAG_INTERNAL instead of hanging.)
    // (Dealing the prologue workgroups only to the XCDs the chain workgroups leave room on was measured and is
    // worse: those are the XCDs of the heaviest batches, whose workgroups then lose their CU to themselves --
    // chain kernel 53.5 us against 41.4 with the prologue spread over all eight.)
    // (sblocks = 8 x rows; a row holds sna sort workgroups and 8 - sna prologue items)
    pa.lead = (pa.sblocks / 8 * pa.sna + pa.ublocks + pa.tblocks + 7) / 8 * 8;
    if (pa.lead < pa.sblocks) pa.lead = pa.sblocks;
    pa.nchain = (int)hp.crefs.size();
    if (c.NL == 1) {
        // (two workgroups per CU by registers and LDS; D = 256: one)
        const int slots = (D == 256 || (c.P->flags & MPQE_STEP_EIGHT_WAVES)) ? STEP_CUS : 2 * STEP_CUS;
#ifdef MPQE_EMU
        const bool fits = false && slots;       // (the host emulator runs a launch's workgroups one after the other, in order)
#else
        // (the placement grid's holes leave at once: only the real chain workgroups hold slots)
        const bool fits = pa.sblocks + hp.blk_off[nb] + 32 <= slots;
#endif
        const int force = mpqe_dbg_value("PROLOGUE_LAST", -1);       // (timing experiments)
        pa.plast = fits && hp.pl_na > 0 && (force >= 0 ? force != 0 : pa.lead > slots / 2) ? 1 : 0;
        if (pa.plast) {
            pa.plna = hp.pl_na; pa.plxrank = 0;
            for (int x = 0; x < STEP_XCDS; ++x) pa.plxrank |= (unsigned)(hp.pl_rank[x] + 1) << (4 * x);
            const int held = pa.sblocks / 8 * (8 - pa.sna);          // items the sort rows hold
            const int rest = pa.ublocks + pa.tblocks > held ? pa.ublocks + pa.tblocks - held : 0;
            pa.lead = pa.sblocks + (rest + pa.plna - 1) / pa.plna * 8;
        }
    }
    // (mpqe_step_extra_t.xcd_shift: idle workgroups in front of the chain workgroups move every one of them that many
    // XCDs on -- forward-only steps on several streams at once)
    if (!c.backward && c.extra && c.extra->xcd_shift > 0 && c.extra->xcd_shift < STEP_XCDS && !pa.plast && pa.sblocks == 0)
        pa.lead += c.extra->xcd_shift;
    if (dbg_on("DUMP_PLAN"))
        fprintf(stderr, "launch: sort rows %d (x8) | pre-pass %d transposes %d | lead %d | chain %d of %d | prologue behind the chain %d (XCDs %d)\n",
                pa.sblocks / 8, pa.ublocks, pa.tblocks, pa.lead, hp.blk_off[nb], pa.nchain, pa.plast, pa.plna);
    pa.slots = at<const WtSlot>(c.db, hp.o_wtslots); pa.WT = c.WT; pa.wt_count = c.epoch_f + 32;
    pa.late = dbg_on("HANDOFF_LATE") ? 1 : 0; pa.fwd_done = c.merged && pa.ublocks > 0 ? c.epoch_f + 33 : nullptr;
    pa.ua.vt_through = c.merged ? 1 : 0;
    if (c.use_runs) pa.runs_count = at<int>(c.wb, hp.o_runs) + hp.touch_M;
    return wt_all;
}
// assemble -> levels -> scores (-> levels back -> anchor-table gradients): the chain workgroups' arguments
static void chain_args(const StepCtx &c, const PrepArgs &pa, int wt_all, ChainArgs &ca) {
    const HostPlan &hp = *c.hp;
    char *db = c.db, *wb = c.wb;
    ca.refs = at<const ChainRef>(db, hp.o_cref); ca.ops = at<const ChainOp>(db, hp.o_cops);
    ca.node_map = c.nm; ca.map_len = (long long)c.P->node_map_len;
    ca.mode_emb = c.P->mode_emb; ca.num_modes = (long long)c.P->num_modes;
    ca.anchor_ids = c.ids; ca.targets = c.tg; ca.negs = c.ng;
    ca.H = c.H; ca.GH = c.GH; ca.WT = c.WT; ca.VT = c.VT;
    ca.epoch_f = c.epoch_f; ca.epoch_b = c.epoch_b;
    ca.DG = c.use_touch ? at<float>(wb, hp.o_DG) : nullptr;
    // (a plan built at pack time also holds the id -> table row hop of every entry; a step that builds its own plan
    // resolves the ids itself)
    ca.erow = c.use_touch && !c.build_touch ? reinterpret_cast<const int *>(reinterpret_cast<const char *>(c.touch) +
                                                                            touch_layout(hp.touch_M, 0).erow) : nullptr;
    ca.Manchor = (long long)hp.anchor_off[c.nb]; ca.Gtot = hp.sd.graphs_total; ca.level_stride = hp.level_stride;
    ca.parts = c.parts; ca.block_terms = at<float>(wb, hp.o_bterms);
    ca.margin = c.margin; ca.eps = 1e-8f;
    ca.s_pos = c.spos; ca.s_neg = c.sneg; ca.terms = c.terms;
    ca.q_out = c.extra ? c.extra->query_out : nullptr;
    ca.err = c.err; ca.backward = c.backward ? 1 : 0;
    ca.stamps = g_chain_stamps && 2 * hp.crefs.size() + (size_t)hp.ts_blocks <= g_chain_stamp_blocks ? g_chain_stamps : nullptr;
    ca.cb = 0; ca.nchain = pa.nchain;
    ca.cv_gran = pa.ublocks > 0 ? at<const unsigned long long>(db, hp.o_gran) : nullptr;
    ca.wt_count = pa.tblocks > 0 ? pa.wt_count : nullptr; ca.wt_blocks = wt_all;
    // (counters and their epoch advance on merged steps only: targets are epoch x count)
    ca.done = c.merged ? at<unsigned>(db, hp.o_done) : nullptr;
    ca.arrive = ca.done ? ca.done + hp.done_inc.size() : nullptr; ca.done_inc = at<const int>(db, hp.o_done_inc);
    ca.ro = hp.ro_chain ? 1 : 0; ca.wt_early = hp.ro_chain && c.P->readout == MPQE_READOUT_CONCAT ? 1 : 0;
    ca.ro_layer = hp.ro_layer; ca.ro_scatter = c.P->readout_scatter;
}
// merged tail: the weight-gradient tiles, the backward post-pass and the zero fill as roles behind the chain workgroups.
// Returns the workgroups of the whole launch (pa.strail apart).
static long long merged_post_args(const StepCtx &c, const PrepArgs &pa, long long zblocks, PostArgs &po) {
    const HostPlan &hp = *c.hp;
    unsigned *done = at<unsigned>(c.db, hp.o_done);
    const int zeroed = (c.P->flags & MPQE_STEP_ZERO_GRADS) ? 1 : 0;
    po.zpad = (int)((zblocks + 7) / 8 * 8);
    if (po.zpad == 0) po.zpad = 8;              // (> 0 marks the merged launch)
    po.zmblocks = zeroed ? (int)hp.zmats.size() * c.ta.zper : 0; po.ublocks = c.ub.nops * c.ub.chunks;
    po.na = hp.post_na; po.xrank = 0;
    for (int x = 0; x < STEP_XCDS; ++x) po.xrank |= (unsigned)(hp.post_rank[x] + 1) << (4 * x);
    po.ppad = (po.zmblocks + po.ublocks + po.na - 1) / po.na * po.na;
    po.wblocks = hp.wblocks_total; po.wblock = c.ta.wblock; po.tile_n = hp.tile_n;
    po.zmats = c.ta.zmats; po.zper = c.ta.zper; po.D = c.D; po.zeroed = zeroed;
    po.ub = c.ub;
    po.ub.done = done; po.ub.done_inc = at<const int>(c.db, hp.o_done_inc); po.ub.dm = hp.dm;
    po.ub.fwd_done = pa.fwd_done; po.ub.fwd_blocks = pa.ublocks; po.ub.epoch_m = c.epoch_f + 48;
    po.slabs = c.slabs; po.H = c.H; po.GH = c.GH; po.level_stride = hp.level_stride; po.gp = c.gp;
    po.done = done; po.done_inc = po.ub.done_inc; po.epoch_m = c.epoch_f + 48;
    po.err = c.err;
    po.stamps = g_tail_stamps && (size_t)po.wblocks <= g_tail_stamp_blocks ? g_tail_stamps : nullptr;
    return pa.lead + pa.nchain + po.zpad + (long long)(po.ppad + po.wblocks + po.na - 1) / po.na * 8;       // (8 workgroups per `na` items)
}
template <int NCB, int KS, int NW = 4, bool RO = false>
static void launch_chain_as(const StepCtx &c, dim3 grid, const ChainArgs &ca, const PrepArgs &pa, const PostArgs &po, const FinArgs &fin) {
    if (fin.count)
        hipLaunchKernelGGL((step_chain_fwd_kernel<NCB, KS, NW, RO>), grid, dim3(64 * NW), 0, c.s, c.sd, c.lp, c.tabs, ca, pa, po, fin);
    else
        hipLaunchKernelGGL((step_chain_kernel<NCB, KS, NW, RO>), grid, dim3(64 * NW), 0, c.s, c.sd, c.lp, c.tabs, ca, pa, po);
}
// what rode in the chain launch and needs no launch behind it: the loss (epoch advance, notification), the readout's regulariser
struct ChainDone { bool loss, reg; };
// the chain launch, bracketed by an event pair: prologue roles, chain workgroups, and behind them the zero fill, the merged
// tail and (forward only) the loss
static ChainDone launch_chain(StepCtx &c, PrepArgs &pa, long long zblocks) {
    const HostPlan &hp = *c.hp;
    const int D = c.D;
    ChainDone did = {false, false};
    const int wt_all = chain_prologue(c, pa);
    ChainArgs ca;
    chain_args(c, pa, wt_all, ca);
    if (ca.stamps && c.build_touch) pa.ts.stamps = g_chain_stamps + 16 * (long long)hp.crefs.size();     // (behind the chain entries)
    PostArgs po;
    memset(&po, 0, sizeof(po));
    long long grid_blocks = pa.lead + pa.nchain + zblocks;
    // (split tail: the untouched relation matrices' zero fill rides behind the chain workgroups; mpqe_debug_option
    // ZMATS_IN_TAIL = 1: by workgroups of the weight-gradient launch, as before)
    if (!c.merged && c.zero_fill && !hp.zmats.empty() && !dbg_on("ZMATS_IN_TAIL")) {
        po.zmblocks = (int)hp.zmats.size() * c.ta.zper;
        po.zmats = c.ta.zmats; po.zper = c.ta.zper; po.D = D; po.gp = c.gp;
        grid_blocks += po.zmblocks;
        c.zmats_in_chain = true;
    }
    if (c.merged) grid_blocks = merged_post_args(c, pa, zblocks, po);
    grid_blocks += pa.strail;
    dim3 cgrid((unsigned)grid_blocks);
    // forward-only: loss, epoch advance and notification by the launch's last workgroup (chain_finish) instead of a
    // launch behind it. mpqe_debug_option LOSS_LAUNCH = 1: step_loss_kernel as before
    FinArgs fin;
    memset(&fin, 0, sizeof(fin));
    if (!c.backward && c.NL == 1 && !dbg_on("LOSS_LAUNCH")) {
        fin.count = c.epoch_f + 42; fin.epoch_f = c.epoch_f; fin.bump_b = pa.tblocks > 0 ? 1 : 0;
        fin.loss = c.loss; fin.bterms = c.bterms; fin.lm = c.lm;
        fin.notify = c.notify; fin.notify_value = c.notify_value; fin.err = c.err;
        did.loss = true;
        if (c.learned && c.extra && c.extra->readout_norms && c.P->readout_weight_decay > 0.f) {
            float wsum = 0.f;
            for (int i = 0; i < c.nb; ++i) wsum += hp.sd.b[i].weight;
            fin.reg_norms = c.extra->readout_norms; fin.reg_coef = c.P->readout_weight_decay * wsum;
            did.reg = true;
        }
    }
    mark(c, c.s);
    if (hp.ro_chain) {
        // (a learned readout on the chain: its own instances -- the others' code stays as it was)
        if (D == 64) launch_chain_as<1, 1, 4, true>(c, cgrid, ca, pa, po, fin);
        else if (D == 128 && (c.P->flags & MPQE_STEP_NO_KSPLIT)) launch_chain_as<2, 1, 4, true>(c, cgrid, ca, pa, po, fin);
        else if (D == 128) launch_chain_as<4, 2, 4, true>(c, cgrid, ca, pa, po, fin);
        else launch_chain_as<4, 1, 4, true>(c, cgrid, ca, pa, po, fin);
    } else if (D == 64) launch_chain_as<1, 1>(c, cgrid, ca, pa, po, fin);
    else if (D == 128 && (c.P->flags & MPQE_STEP_NO_KSPLIT)) launch_chain_as<2, 1>(c, cgrid, ca, pa, po, fin);
    else if (D == 128 && (c.P->flags & MPQE_STEP_EIGHT_WAVES)) launch_chain_as<2, 2, 8>(c, cgrid, ca, pa, po, fin);
    else if (D == 128) launch_chain_as<4, 2>(c, cgrid, ca, pa, po, fin);
    else launch_chain_as<4, 1>(c, cgrid, ca, pa, po, fin);
    mark(c, c.s);
    return did;
}
static int run_chain_form(StepCtx &c) {
    PrepArgs pa;
    memset(&pa, 0, sizeof(pa));
    long long zblocks = 0;
    if (c.zero_fill) {
        // (SPARSE_TABLES: only the touched rows of the table gradients are ever read; they are written, not accumulated)
        if (!c.use_touch && !c.sparse_tables) {
            // chain form WITHOUT a touch plan: the chain workgroups add into the tables with atomics -- a zero fill inside
            // their own launch would race with them: a launch of its own in front
            ZeroSegs zt;
            memset(&zt, 0, sizeof(zt));
            long long ztb = 0;
            for (int m = 0; m < c.P->num_modes; ++m) zero_seg(zt, ztb, c.G->tables[m], (long long)c.P->table_rows[m] * c.D);
            zt.block0[zt.count] = ztb;
            if (ztb > 0) hipLaunchKernelGGL(step_zero_kernel, dim3((unsigned)ztb), dim3(256), 0, c.s, zt);
        }
        zblocks = grad_zero_segs(c, pa.zs, c.use_touch && !c.sparse_tables);     // (the rest: workgroups of the chain launch)
    }
    fork_lanes(c);
    const ChainDone did = launch_chain(c, pa, zblocks);
    if (!c.backward) {
        join_lanes(c);
        if (!did.loss) launch_loss(c, pa.tblocks > 0 ? 1 : 0);
        if (c.learned && !did.reg) ro_regulariser(c, false);
        return mpqe_launch_status();
    }
    // (a side stream for the post-pass / table rows beside the tiles was measured: the cross-stream fork and join
    // cost more than the overlap gains -- 93.8 us per step against 81.8 with everything on one stream)
    mark(c, c.s);
    if (!c.merged) launch_grad_w(c, c.s);
    mark(c, c.s);
    join_lanes(c);
    launch_reduce(c);
    if (c.learned) ro_regulariser(c, true);
    return mpqe_launch_status();
}

// ------------------------------------------------------------------------------------ level form
// learned readouts off the chain: gather -> Linear - ReLU - Linear -> reduction over each graph's rows, and the way back;
// the caller's readout: its embeddings and their gradients
struct LevelReadout {
    RoArgs roa;
    float *x, *gx, *h, *y, *gy, *gh;
    const float *Qc;
    float *GQc;
};
static LevelReadout level_readout(const StepCtx &c) {
    const HostPlan &hp = *c.hp;
    LevelReadout ro;
    memset(&ro, 0, sizeof(ro));
    ro.Qc = c.P->readout == MPQE_READOUT_CALLER ? at<const float>(c.wb, hp.o_Q) : nullptr;
    ro.GQc = c.P->readout == MPQE_READOUT_CALLER ? at<float>(c.wb, hp.o_GQ) : nullptr;
    ro.roa.kind = c.P->readout; ro.roa.op = c.P->readout_scatter;
    ro.roa.mrows = hp.ro_rows; ro.roa.kin = hp.ro_kin; ro.roa.level_stride = hp.level_stride;
    if (c.learned) {
        const long long lv = (long long)hp.sd.b[0].L * hp.level_stride;
        ro.x = hp.ro_direct ? c.H + lv : at<float>(c.wb, hp.o_rx); ro.gx = hp.ro_direct ? c.GH + lv : at<float>(c.wb, hp.o_rgx);
        ro.h = at<float>(c.wb, hp.o_rh); ro.gh = at<float>(c.wb, hp.o_rgh);
        ro.y = at<float>(c.wb, hp.o_ry); ro.gy = at<float>(c.wb, hp.o_rgy);
    }
    return ro;
}
static dim3 ro_blocks(long long threads) { return dim3((unsigned)((threads + 255) / 256)); }
static int ro_forward(const StepCtx &c, const LevelReadout &ro) {
    const RoArgs &roa = ro.roa;
    if (!c.hp->ro_direct)
        hipLaunchKernelGGL(step_ro_gather_kernel, ro_blocks(roa.mrows * (roa.kin / 4)), dim3(256), 0, c.s, c.sd, roa,
                           (const float *)c.H, ro.x);
    const int st = mpqe_linear_fwd(ro.x, roa.mrows, c.P->readout_w0, roa.kin, c.P->readout_b0, roa.kin, c.D, 1, 0, ro.h, c.s);
    if (st) return st;
    // (the reduction over each graph's rows: inside the score kernel)
    return mpqe_linear_fwd(ro.h, roa.mrows, c.P->readout_w2, c.D, c.P->readout_b2, c.D, c.D, 0, 0, ro.y, c.s);
}
static int ro_backward(const StepCtx &c, const LevelReadout &ro) {
    const HostPlan &hp = *c.hp;
    const RoArgs &roa = ro.roa;
    const int D = c.D;
    void *lw = c.wb + hp.o_rlin;         // (the score kernel has written the rows' gradients)
    int st = mpqe_linear_bwd(ro.h, roa.mrows, c.P->readout_w2, D, ro.y, ro.gy, D, D, 0, 0, ro.gh, c.G->readout_w2, D,
                             c.G->readout_b2, lw, hp.rlin_bytes, c.s);
    if (st) return st;
    st = mpqe_linear_bwd(ro.x, roa.mrows, c.P->readout_w0, roa.kin, ro.h, ro.gh, roa.kin, D, 1, 0, ro.gx,
                         c.G->readout_w0, roa.kin, c.G->readout_b0, lw, hp.rlin_bytes, c.s);
    if (st) return st;
    if (!hp.ro_direct)
        hipLaunchKernelGGL(step_ro_spread_kernel, ro_blocks(hp.sd.rows_total * (D / 4)), dim3(256), 0, c.s, c.sd, roa,
                           (const float *)ro.gx, c.GH);
    return MPQE_OK;
}
static void launch_assemble(const StepCtx &c, int l) {
    const long long nr = c.row0[l + 1] - c.row0[l], ngr = c.gr0[l + 1] - c.gr0[l];
    const long long waves = nr + 2 * ngr;
    int lpr_h = c.vec_tab ? 1 : 64;        // lanes per row
    while (lpr_h < 64 && lpr_h * 4 < c.D) lpr_h <<= 1;
    const long long per_block = 4 * (64 / lpr_h);
    hipLaunchKernelGGL(step_assemble_kernel, dim3((unsigned)((waves + per_block - 1) / per_block)), dim3(256), 0, c.ls[l], c.sd,
                       c.tabs, c.nm, (long long)c.P->node_map_len, c.P->mode_emb, (long long)c.P->num_modes, c.ids, c.tg, c.ng, c.H,
                       c.tpos, c.tneg, c.err, c.vec_tab, c.row0[l], nr, c.gr0[l], ngr);
}
// level p of lane l, forward / backward-x, bracketed by an event pair on the lane's stream
template <int MODE>
static void launch_layer_fwd_as(const StepCtx &c, int l, int p) {
    const HostPlan &hp = *c.hp;
    hipLaunchKernelGGL(step_layer_fwd_kernel<MODE>, dim3((unsigned)hp.tfwd[l][p].size()), dim3(256), 0, c.ls[l], c.sd, c.lp, p,
                       at<const TileRef>(c.db, hp.o_tf[l][p]), (const float *)(c.H + (long long)p * hp.level_stride),
                       c.H + (long long)(p + 1) * hp.level_stride);
}
static void launch_layer_fwd(StepCtx &c, int l, int p) {
    mark(c, c.ls[l]);
    if (c.fast) launch_layer_fwd_as<LD_FAST>(c, l, p);
    else if (c.vec) launch_layer_fwd_as<LD_PRED>(c, l, p);
    else launch_layer_fwd_as<LD_SCALAR>(c, l, p);
    mark(c, c.ls[l]);
}
// readout + cosine scores + hinge terms of lane l's graphs (BWD: and the rows of gH[L_b], the targets' / negatives' table rows)
template <bool BWD, int NJ>
static void launch_score_as(const StepCtx &c, const LevelReadout &ro, int l) {
    const long long ngr = c.gr0[l + 1] - c.gr0[l];
    hipLaunchKernelGGL((step_score_kernel<BWD, NJ>), dim3((unsigned)((ngr + 3) / 4)), dim3(256), 0, c.ls[l], c.sd, (const float *)c.H,
                       c.hp->level_stride, (const float *)c.tpos, (const float *)c.tneg, c.margin, 1e-8f, c.spos, c.sneg, c.terms,
                       BWD ? c.GH : (float *)nullptr, c.tabs, c.nm, (long long)c.P->node_map_len, c.tg, c.ng, c.gr0[l], ngr,
                       ro.Qc, ro.GQc, (const float *)(c.learned ? ro.y : nullptr), c.learned ? ro.gy : (float *)nullptr, ro.roa.op);
}
template <bool BWD>
static void launch_score(const StepCtx &c, const LevelReadout &ro, int l) {
    if (c.D <= 64) launch_score_as<BWD, 1>(c, ro, l);
    else if (c.D <= 128) launch_score_as<BWD, 2>(c, ro, l);
    else if (c.D <= 256) launch_score_as<BWD, 4>(c, ro, l);
    else launch_score_as<BWD, 8>(c, ro, l);
}
static void launch_scores(const StepCtx &c, const LevelReadout &ro, bool bwd) {      // every lane's, on its stream
    for (int l = 0; !bwd && l < c.NL; ++l) launch_score<false>(c, ro, l);
    for (int l = 0; bwd && l < c.NL; ++l) launch_score<true>(c, ro, l);
}
template <int MODE>
static void launch_layer_bwd_x_as(const StepCtx &c, int l, int p) {
    const HostPlan &hp = *c.hp;
    hipLaunchKernelGGL(step_layer_bwd_x_kernel<MODE>, dim3((unsigned)hp.tbwd[l][p].size()), dim3(256), 0, c.ls[l], c.sd, c.lp, p,
                       at<const TileRef>(c.db, hp.o_tb[l][p]), (const float *)(c.GH + (long long)(p + 1) * hp.level_stride),
                       (const float *)(c.H + (long long)p * hp.level_stride), c.GH + (long long)p * hp.level_stride, c.add_states);
}
static void launch_layer_bwd_x(StepCtx &c, int l, int p) {
    mark(c, c.ls[l]);
    if (c.fast) launch_layer_bwd_x_as<LD_FAST>(c, l, p);
    else if (c.vec) launch_layer_bwd_x_as<LD_PRED>(c, l, p);
    else launch_layer_bwd_x_as<LD_SCALAR>(c, l, p);
    mark(c, c.ls[l]);
}
static int run_level_form(StepCtx &c) {
    const HostPlan &hp = *c.hp;
    if (c.zero_fill) {       // the gradients' zero fill: a launch of its own
        ZeroSegs zs;
        memset(&zs, 0, sizeof(zs));
        const long long zblocks = grad_zero_segs(c, zs, !c.sparse_tables);
        if (zblocks > 0) hipLaunchKernelGGL(step_zero_kernel, dim3((unsigned)zblocks), dim3(256), 0, c.s, zs);
    }
    fork_lanes(c);
    const LevelReadout ro = level_readout(c);
    // ---- forward
    if (!c.phase_bwd && !c.phase_score) {
        for (int l = 0; l < c.NL; ++l) launch_assemble(c, l);
        for (int p = 0; p < hp.Lmax; ++p)
            for (int l = 0; l < c.NL; ++l)
                if (p < hp.lane_Lmax[l]) launch_layer_fwd(c, l, p);
    }
    if (c.phase_fwd) return mpqe_launch_status();     // the node states of every level are in the workspace (mpqe_step_states_layout)
    if (c.learned) {
        const int st = ro_forward(c, ro);
        if (st) return st;
    }
    if (!c.backward) {
        launch_scores(c, ro, false);
        join_lanes(c);
        launch_loss(c, 0);
        if (c.learned) ro_regulariser(c, false);
        return mpqe_launch_status();
    }
    // ---- backward (the score kernel's backward instance writes scores and hinge terms too; the loss
    // itself is reduced by the last launch of the step)
    // (the caller's readout: its own call for the scores -- embeddings in, their gradients out --, then the caller writes the
    // rows of gH[L_b] and the last call takes it from there)
    if (!c.phase_bwd) launch_scores(c, ro, true);
    if (c.phase_score) return mpqe_launch_status();
    if (c.learned) {
        const int st = ro_backward(c, ro);
        if (st) return st;
    }
    for (int p = hp.Lmax - 1; p >= 0; --p)
        for (int l = 0; l < c.NL; ++l)
            if (p < hp.lane_Lmax[l]) launch_layer_bwd_x(c, l, p);
    join_lanes(c);
    mark(c, c.s);
    launch_grad_w(c, c.s);
    mark(c, c.s);
    // bias / variable-row partials and anchor-table gradients (the chain kernel does them itself)
    const unsigned small_blocks = (unsigned)(c.ta.vblocks + (hp.anchor_off[c.nb] + 3) / 4);
    if (small_blocks)
        hipLaunchKernelGGL(step_tail_small_kernel, dim3(small_blocks), dim3(256), 0, c.s, c.sd, c.ta, c.tabs, (const float *)c.H,
                           (const float *)c.GH, hp.level_stride);
    launch_reduce(c);
    if (c.learned) ro_regulariser(c, true);
    return mpqe_launch_status();
}

static int step_ex(const StepCall &call) {
    // (what the plan lookup itself reads; every other check: step_check)
    if (!call.P || !call.B || call.nb < 1 || call.nb > MPQE_STEP_MAX_BATCHES || !call.desc) return MPQE_ERR_INVALID_ARG;
    StepCtx c{};
    static_cast<StepCall &>(c) = call;
    int st = plan_lookup(call.P, call.B, call.nb, call.lanes, call.desc, &c.upload_desc, &c.cached);
    if (st) return st;
    c.hp = &c.cached->hp;
    step_flags(c);
    st = step_check(c);
    if (st) return st;
    step_resolve(c);
    queue_descriptors(c);
    step_launch_args(c);
    return c.chain ? run_chain_form(c) : run_level_form(c);
}

extern "C" int mpqe_step_forward_backward_ex(const mpqe_step_params_t *P, const mpqe_step_batch_t *B, int nb,
                                             const int64_t *anchor_ids, const int64_t *targets, const int64_t *negs,
                                             float margin, const mpqe_step_grads_t *G, int backward,
                                             float *loss, float *scores_pos, float *scores_neg, void *desc,
                                             size_t desc_bytes, int upload_desc, void *workspace,
                                             size_t workspace_bytes, int32_t *err, const mpqe_step_lanes_t *lanes,
                                             void *const *events, int num_events, void *touch, void *stream,
                                             const mpqe_step_extra_t *extra) {
    const StepCall call = {P, B, nb, anchor_ids, targets, negs, margin, G, backward, loss, scores_pos, scores_neg, desc, desc_bytes,
                           upload_desc, workspace, workspace_bytes, err, lanes, events, num_events, touch, stream, extra};
    const int st = step_ex(call);
    // (mpqe_step_extra_t.join_event / join_stream: the consumer's stream waits for this call's launches)
    if (st == MPQE_OK && extra && extra->join_event && extra->join_stream != stream) {
        if (hipEventRecord(reinterpret_cast<hipEvent_t>(extra->join_event), as_stream(stream)) != hipSuccess ||
            hipStreamWaitEvent(as_stream(extra->join_stream), reinterpret_cast<hipEvent_t>(extra->join_event), 0) != hipSuccess)
            return MPQE_ERR_LAUNCH;
    }
    return st;
}
