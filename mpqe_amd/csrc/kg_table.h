// The KG index as ONE device table (include/mpqe_amd.h: mpqe_kg_table_build): what a kernel needs to follow a relation
// INDEX it finds in a query's own record -- the kernels of kg.hip / kg_sample.hip before it take their relations from the
// host, one formula a launch. Built once per index by the host and copied; read-only afterwards.
//   KgtHead | KgtRel [num_rels]
#pragma once
#include "common.h"

#define KGT_MAX_RELS 4096
#define KGT_MAX_MODES 16
#define KGT_MAGIC 0x4b475437            // a table that was never built is refused by the kernels (flagged), not followed

struct KgtHead {
    int num_rels, num_modes, magic, pad;
    long long mode_rows[KGT_MAX_MODES];
    const uint32_t *valid[KGT_MAX_MODES];       // [W(mode)]: the rows that are entities; NULL: every row below n
    const long long *row_ids[KGT_MAX_MODES];    // [n]: row -> entity id; NULL: none given
};

struct KgtRel {
    const long long *off;       // [n_src + 1]
    const long long *rows;      // [edges], rows of the destination mode
    long long edges;
    int n_src, n_dst, src, dst;
    int reverse, pad;           // the index of reverse_relation(rel) in the same index, -1: absent
};

// The host's copy of the modes, checked as the mixed entry points take it: the widest mode's rows; 0 for no modes, more than
// the table holds or a mode without a row. (How wide a mode may be is the caller's own limit.)
static inline int64_t kgt_widest_mode(const int64_t *mode_rows, int num_modes) {
    if (!mode_rows || num_modes < 1 || num_modes > KGT_MAX_MODES) return 0;
    int64_t widest = 0;
    for (int m = 0; m < num_modes; ++m) {
        if (mode_rows[m] < 1) return 0;
        if (mode_rows[m] > widest) widest = mode_rows[m];
    }
    return widest;
}

__device__ __forceinline__ const KgtHead *kgt_head(const char *table) { return reinterpret_cast<const KgtHead *>(table); }
__device__ __forceinline__ const KgtRel *kgt_rels(const char *table) {
    return reinterpret_cast<const KgtRel *>(table + sizeof(KgtHead));
}
