"""Exact answers of conjunctive queries on the knowledge graph, on the device (csrc/kg.hip; include/mpqe_amd.h:
mpqe_kg_answers, mpqe_kg_rows). The reference keeps this as Python sets (Graph.get_metapath_neighs graph.py:459-473,
Graph.get_negative_samples graph.py:263-314); here the graph is one CSR per typed relation in HBM, a set of entities is a
bitmap over a mode's TABLE ROWS (node_maps[id], the row space of ops.rank_entities), and a batch of queries of one formula
is one launch.

    index = KGIndex.from_graph(graph, enc.node_maps, device)           # once; or KGIndex.from_edges(...) from arrays
    ans = index.answers(formula, queries, hard=True)                   # KGAnswers: bits / hard_bits / counts on the device
    model.rank_targets(formula, queries, targets, exclude=ans)         # filtered ranking without host lists
    eval_rank_queries(test_queries, model, known_answers=index)
    NegativeSampler.from_csr(ans.negative_csr(), ans.hard_csr(), device)

Sampling on the index (csrc/kg_sample.hip: mpqe_kg_sample_queries, mpqe_kg_sample_rows; reference Graph.sample_queries /
sample_test_queries graph.py:227-260, sample_query_subgraph_bytype graph.py:321-389, Query(neg_sample_max) graph.py:83-87):

    records = index.sample_queries('3-inter', 100000, seed)            # [count, 10] int64 on the device: the walk
    ans.sample_negative_csr(100, seed), ans.sample_hard_csr(100, seed) # at most 100 negatives a query, on the device
    sets = index.sample_query_sets(['2-chain', '3-inter'], 10000, seed, train_index=None)      # {Formula: QuerySet}
    sets[f].negative_sampler(); sets[f].queries()

Queries of DIFFERENT formulas in one launch (mpqe_kg_answers_mixed, mpqe_kg_sample_rows_mixed; the relations come from every
query's own record, through a device table of the index built once):

    mixed = index.answers_mixed('3-inter', records, hard=True)         # KGAnswersMixed: counts, target_mode, member, bits
    mixed.sample_negative_csr(100, seed), mixed.sample_hard_csr(100, seed)
    sets = index.sample_query_sets(types, 10000, seed, batched=True)   # a cost per type, not per formula
"""
import contextlib
import ctypes
import time

import numpy as np
import torch

from . import _capi, ops
from .graph import Formula, Query, reverse_relation

PROG_INTS = ops.GQE_PROG_INTS
MAX_MODES = 16

# The seven query types in query EDGES (x, rel, y), in the order of the reference's query tuple and of sample_queries' records:
# (edges, the anchor edges -- their y is the anchor -- in anchor-slot order, the variable edges, whether Formula nests the
# relations as (r0, (r1, r2))). Edge 0's x is the target.
QUERY_SHAPES = {
    '1-chain': (1, (0,), (), False),
    '2-chain': (2, (1,), (0,), False),
    '3-chain': (3, (2,), (0, 1), False),
    '2-inter': (2, (0, 1), (), False),
    '3-inter': (3, (0, 1, 2), (), False),
    '3-inter_chain': (3, (0, 2), (1,), True),
    '3-chain_inter': (3, (1, 2), (0,), True),
}


def _edge_relations(formula):
    """the formula's relations, one per query edge in QUERY_SHAPES' edge order"""
    rels = formula.rels
    return [tuple(r) for r in ((rels[0],) + tuple(rels[1]) if QUERY_SHAPES[formula.query_type][3] else rels)]


def query_hops(formula):
    """([(anchor slot, [relation of each hop])], [relations of the hops after the merge]): the walk from the anchors to the
    target. A query edge (x, rel, y) is walked from y to x along reverse_relation(rel), whose CSR lists the x of a y
    (synthetic._answers; reference graph.py:266, 274, 290, 300-307)."""
    qt, rels = formula.query_type, formula.rels
    rev = reverse_relation
    if qt.endswith('-chain'):
        return [(0, [rev(tuple(r)) for r in reversed(rels)])], []
    if qt.endswith('-inter'):
        return [(i, [rev(tuple(r))]) for i, r in enumerate(rels)], []
    if qt == '3-inter_chain':
        return [(0, [rev(tuple(rels[0]))]), (1, [rev(tuple(rels[1][1])), rev(tuple(rels[1][0]))])], []
    if qt == '3-chain_inter':
        return [(0, [rev(tuple(rels[1][0]))]), (1, [rev(tuple(rels[1][1]))])], [rev(tuple(rels[0]))]
    raise ValueError('unknown query type %r' % (qt,))


def kg_programme(branches, tail, target_mode):
    """The int32 programme of mpqe_kg_answers: the layout of ops.gqe_programme with code = relation << 4 | destination mode.
    branches: [(anchor mode, [(relation index, destination mode)])], tail: [(relation index, destination mode)]."""
    prog = np.full(PROG_INTS, -1, dtype=np.int32)
    prog[0], prog[1], prog[2], prog[5], prog[6], prog[7] = 1, len(branches), 0, len(tail), target_mode, 0
    for b, (mode, steps) in enumerate(branches):
        prog[8 + 5 * b], prog[9 + 5 * b] = mode, len(steps)
        for s, (rel, dst) in enumerate(steps):
            prog[10 + 5 * b + s] = (rel << 4) | dst
    for s, (rel, dst) in enumerate(tail):
        prog[24 + s] = (rel << 4) | dst
    return prog


def _words(n):
    return (int(n) + 31) // 32


def _bitmap(rows, n):
    """uint32 words of the set `rows` of a mode with n rows (bit r % 32 of word r / 32), as int32 for torch."""
    flags = np.zeros(_words(n) * 32, dtype=np.uint8)
    flags[np.asarray(rows, dtype=np.int64)] = 1
    return np.packbits(flags, bitorder='little').view(np.uint32).view(np.int32)


def _unpack(words, n):
    """[Q, W] words -> one ascending array of rows per query"""
    words = np.ascontiguousarray(words).view(np.uint32)
    flags = np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder='little')[:, :n]
    return [np.nonzero(f)[0].astype(np.int64) for f in flags]


class KGIndex(object):
    """The graph on the device: per typed relation a CSR over table rows, per mode its row count n (1 + the last row
    that is an entity, as _EntityRanking._mode_rows has it), the row -> id map and the bitmap of the rows that are
    entities. Built once. lib: a bound C-ABI library to call instead of the product's -- the tests run a CPU-resident index
    on the host emulator of the kernels; without one the index must live on the GPU (there is no CPU path)."""

    def __init__(self, mode_ids_of, edges, node_maps, device, lib=None):
        self.device = torch.device(device)
        self.lib = lib
        maps = node_maps.detach().cpu().numpy() if torch.is_tensor(node_maps) else np.asarray(node_maps)
        self.maps_host = maps = np.ascontiguousarray(maps, dtype=np.int64)
        self.modes = list(mode_ids_of)
        if not 1 <= len(self.modes) <= MAX_MODES:
            raise ValueError('KGIndex: 1 to %d modes, got %d' % (MAX_MODES, len(self.modes)))
        self.mode_index = {m: i for i, m in enumerate(self.modes)}
        self.row_ids_host, self.row_ids, self.valid, self.num_entities = {}, {}, {}, {}
        mode_rows = []
        for m in self.modes:
            ids = np.asarray(list(mode_ids_of[m]), dtype=np.int64)
            if ids.size == 0 or ids.min() < 0 or ids.max() >= maps.shape[0]:
                raise IndexError('KGIndex: mode %r is empty or holds ids outside node_maps' % (m,))
            rows = maps[ids]
            if rows.min() < 0:
                raise IndexError('KGIndex: mode %r holds ids without a table row' % (m,))
            n = int(rows.max()) + 1
            row_ids = np.full(n, -1, dtype=np.int64)
            row_ids[rows] = ids
            self.row_ids_host[m] = row_ids
            self.row_ids[m] = torch.from_numpy(row_ids).to(self.device)
            self.valid[m] = torch.from_numpy(_bitmap(np.nonzero(row_ids >= 0)[0], n)).to(self.device)
            self.num_entities[m] = int((row_ids >= 0).sum())
            mode_rows.append(n)
        self.mode_rows = np.asarray(mode_rows, dtype=np.int64)
        self.rels = [tuple(r) for r in edges]
        self.rel_index = {r: i for i, r in enumerate(self.rels)}
        self.offsets, self.rows, self.start_rows = [], [], []
        for rel in self.rels:
            src, dst = edges[rel]
            off, rows = self._csr(rel, np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(dst, dtype=np.int64).reshape(-1))
            self.offsets.append(torch.from_numpy(off).to(self.device))
            self.rows.append(torch.from_numpy(rows).to(self.device))
            self.start_rows.append(torch.from_numpy(np.nonzero(np.diff(off))[0].astype(np.int64)).to(self.device))
        R = max(len(self.rels), 1)
        self._off_arr = (ctypes.c_void_p * R)(*[t.data_ptr() for t in self.offsets])
        self._rows_arr = (ctypes.c_void_p * R)(*[t.data_ptr() if t.numel() else None for t in self.rows])
        self._edges_arr = (ctypes.c_int64 * R)(*[t.numel() for t in self.rows])
        # what the walk takes besides the CSRs: every relation's modes and its source rows that have an edge
        self.rel_src = np.asarray([self.mode_index[r[0]] for r in self.rels] or [0], dtype=np.int32)
        self.rel_dst = np.asarray([self.mode_index[r[2]] for r in self.rels] or [0], dtype=np.int32)
        self._start_arr = (ctypes.c_void_p * R)(*[t.data_ptr() if t.numel() else None for t in self.start_rows])
        self._start_count = (ctypes.c_int64 * R)(*[t.numel() for t in self.start_rows])
        self._programmes = {}
        self._maps_dev = None
        self._table = None
        self.section_times = None       # a dict: sample_query_sets(batched=True) adds its sections' seconds (it then synchronises)
        self.err = ops.new_error_word(self.device)

    @contextlib.contextmanager
    def _call(self):
        """-> (library, stream) for one C-ABI call on this index's device"""
        if self.lib is not None:
            yield self.lib, None
        elif self.device.type != 'cuda':
            raise RuntimeError('mpqe_amd: the KG index must be on a CUDA (ROCm) device -- there is no CPU path')
        else:
            with torch.cuda.device(self.device):
                yield ops.lib(), ops._stream()

    def _rows_of(self, mode, ids):
        """table rows of ids of `mode`; an id of another mode, of no mode or outside node_maps becomes row n (outside)"""
        maps, row_ids = self.maps_host, self.row_ids_host[mode]
        n = row_ids.shape[0]
        inside = (ids >= 0) & (ids < maps.shape[0])
        cand = np.where(inside, maps[np.where(inside, ids, 0)], -1)
        ok = (cand >= 0) & (cand < n)
        ok &= row_ids[np.where(ok, cand, 0)] == ids
        return np.where(ok, cand, n)

    def _csr(self, rel, src, dst):
        if rel[0] not in self.mode_index or rel[2] not in self.mode_index or src.shape != dst.shape:
            raise ValueError('KGIndex: relation %r names an unknown mode or its arrays differ in length' % (rel,))
        n_src, n_dst = self.row_ids_host[rel[0]].shape[0], self.row_ids_host[rel[2]].shape[0]
        s, d = self._rows_of(rel[0], src), self._rows_of(rel[2], dst)
        if (s >= n_src).any() or (d >= n_dst).any():
            raise IndexError('KGIndex: an edge of %r has an endpoint that is no entity of its mode' % (rel,))
        order = np.argsort(s, kind='stable')
        off = np.zeros(n_src + 1, dtype=np.int64)
        np.cumsum(np.bincount(s, minlength=n_src), out=off[1:])
        return off, np.ascontiguousarray(d[order], dtype=np.int64)

    @classmethod
    def from_graph(cls, graph, node_maps, device, lib=None):
        """From graph.adj_lists ({relation: {node: neighbours}}) and graph.full_lists ({mode: ids})."""
        if getattr(graph, 'adj_lists', None) is None:
            raise ValueError('KGIndex.from_graph: the graph has no adjacency (use from_edges)')
        edges = {}
        for rel, adj in graph.adj_lists.items():
            lens = np.fromiter((len(v) for v in adj.values()), dtype=np.int64, count=len(adj))
            src = np.repeat(np.fromiter(adj.keys(), dtype=np.int64, count=len(adj)), lens)
            dst = np.fromiter((x for v in adj.values() for x in v), dtype=np.int64, count=int(lens.sum()))
            edges[tuple(rel)] = (src, dst)
        return cls({m: graph.full_lists[m] for m in graph.full_lists}, edges, node_maps, device, lib)

    @classmethod
    def from_edges(cls, schema_or_modes, edges, node_maps, device, lib=None):
        """From arrays: schema_or_modes is a synthetic.Schema or {mode: ids}; edges {(m1, name, m2): (src ids, dst ids)}.
        A relation and its inverse are two entries (the index holds what it is given)."""
        ids = getattr(schema_or_modes, 'ids', schema_or_modes)
        return cls(ids, edges, node_maps, device, lib)

    # ------------------------------------------------------------------------------------------ queries
    def programme(self, formula):
        hit = self._programmes.get(formula)
        if hit is None:
            branches, tail = query_hops(formula)

            def code(rel):
                if rel not in self.rel_index:
                    raise KeyError('KGIndex: no adjacency for relation %r' % (rel,))
                return self.rel_index[rel], self.mode_index[rel[2]]
            prog = kg_programme([(self.mode_index[steps[0][0]], [code(r) for r in steps]) for _, steps in branches],
                                [code(r) for r in tail], self.mode_index[formula.target_mode])
            hit = self._programmes[formula] = (np.ascontiguousarray(prog), [slot for slot, _ in branches])
        return hit

    def anchor_rows(self, formula, queries_or_anchor_ids):
        """[branches, B] int64 on the device: the table rows of the anchors"""
        _, slots = self.programme(formula)
        a = queries_or_anchor_ids
        if torch.is_tensor(a):
            a = a.detach().cpu().numpy()
        elif len(a) and hasattr(a[0], 'anchor_nodes'):
            a = [q.anchor_nodes for q in a]
        ids = np.asarray(a, dtype=np.int64).reshape(-1, len(formula.anchor_modes))
        rows = np.stack([self._rows_of(formula.anchor_modes[s], ids[:, s]) for s in slots]) if ids.shape[0] else \
            np.zeros((len(slots), 0), dtype=np.int64)
        return torch.from_numpy(np.ascontiguousarray(rows)).to(self.device)

    def answers(self, formula, queries_or_anchor_ids, hard=False, global_bits=False):
        """The exact answer sets of a batch of queries of one formula (Query objects, or anchor ids [B, anchors]) ->
        KGAnswers. hard: also the hard negatives' sets (union of the branches minus the answers)."""
        prog, _ = self.programme(formula)
        rows = self.anchor_rows(formula, queries_or_anchor_ids)
        return self.answers_of_rows(formula, prog, rows, hard, global_bits)

    def answers_of_rows(self, formula, prog, anchor_rows, hard=False, global_bits=False):
        """answers() from its two prepared inputs: the programme and the anchors' rows [branches, B] on the device (nothing
        is translated or uploaded here). global_bits: the working bitmaps in the workspace whatever their size."""
        mode = formula.target_mode
        n = int(self.mode_rows[self.mode_index[mode]])
        Q, W = int(anchor_rows.shape[1]), _words(n)
        dev = self.device
        bits = torch.empty((Q, W), dtype=torch.int32, device=dev)
        hard_bits = torch.empty((Q, W), dtype=torch.int32, device=dev) if hard else None
        counts = torch.empty((2, Q), dtype=torch.int64, device=dev)
        if Q:
            flags = _capi.KG_GLOBAL_BITS if global_bits else 0
            with self._call() as (lib, stream):
                need = lib.mpqe_kg_workspace_bytes(prog.ctypes.data, Q, self.mode_rows.ctypes.data, len(self.modes), flags)
                if need == 0:
                    raise ValueError('KGIndex.answers: programme outside what the kernel covers')
                ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
                _capi.check(lib, lib.mpqe_kg_answers(prog.ctypes.data, self._off_arr, self._rows_arr, self._edges_arr,
                                                     len(self.rels), self.mode_rows.ctypes.data, len(self.modes),
                                                     anchor_rows.data_ptr(), Q, bits.data_ptr(), ops._p(hard_bits),
                                                     counts.data_ptr(), flags, _capi._align256(ws.data_ptr()), need,
                                                     self.err.data_ptr(), stream), 'mpqe_kg_answers')
        return KGAnswers(self, formula, mode, n, bits, hard_bits, counts)

    def check(self):
        """IndexError if a call since the last check met an anchor that is no entity of its mode (its query got empty
        sets). One 4-byte read."""
        ops.raise_on_flags(self.err)

    # ------------------------------------------------------------------------------------------ sampling
    def sample_queries(self, query_type, count, seed, max_tries=8):
        """The reference's random walk (Graph.sample_query_subgraph_bytype) for `count` slots -> [count, 10] int64 on the
        device: status (1 a query, 0 none after max_tries), then up to three edges (source row, relation index, destination
        row) in the order of the reference's query tuple, -1 padded. A pure function of (seed, slot, the index)."""
        qt = _capi.QUERY_TYPE_IDS[query_type] if isinstance(query_type, str) else int(query_type)
        count = int(count)
        out = torch.empty((count, _capi.KG_QUERY_INTS), dtype=torch.int64, device=self.device)
        if count:
            if not self.rels:
                raise ValueError('KGIndex.sample_queries: the index has no relation')
            with self._call() as (lib, stream):
                need = lib.mpqe_kg_sample_workspace_bytes(len(self.rels), len(self.modes))
                if need == 0:
                    raise ValueError('KGIndex.sample_queries: more relations than the walk covers')
                ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
                _capi.check(lib, lib.mpqe_kg_sample_queries(
                    self._off_arr, self._rows_arr, self._edges_arr, self.rel_src.ctypes.data, self.rel_dst.ctypes.data,
                    self._start_arr, self._start_count, len(self.rels), self.mode_rows.ctypes.data, len(self.modes), qt,
                    count, int(max_tries), int(seed) & (2 ** 64 - 1), out.data_ptr(), _capi._align256(ws.data_ptr()), need,
                    self.err.data_ptr(), stream), 'mpqe_kg_sample_queries')
        return out

    def rows_of(self, mode, ids):
        """Table rows of entity ids of `mode`, int64 on the index's device, computed there (ids: a list, an array or a
        tensor). A negative id -- the null node -- stays -1; an id that is no entity of the mode becomes row n (outside,
        which the kernels flag)."""
        ids = torch.as_tensor(ids, dtype=torch.int64).to(self.device).reshape(-1)
        if self._maps_dev is None:
            self._maps_dev = torch.from_numpy(self.maps_host).to(self.device)
        maps, row_ids = self._maps_dev, self.row_ids[mode]
        n = row_ids.shape[0]
        inside = (ids >= 0) & (ids < maps.shape[0])
        cand = torch.where(inside, maps[ids.clamp(0, maps.shape[0] - 1)], torch.full_like(ids, -1))
        ok = (cand >= 0) & (cand < n)
        ok &= row_ids[cand.clamp(0, n - 1)] == ids
        rows = torch.where(ok, cand, torch.full_like(ids, n))
        return torch.where(ids < 0, torch.full_like(ids, -1), rows)

    def sample_neighbours(self, mode, rows, keep_prob=0.5, max_keep=10, seed=0, relations=None, err=None):
        """The draws of the reference's MeanAggregator (aggregators.py:51-53) for a batch of source ROWS of `mode` (device
        int64; rows_of gives them for ids; negative: the null node) and every relation out of the mode, in one launch ->
        (relations, neigh [R, B, max_keep] int64, counts [R, B] int32) on the device. relations: the (mode, name, mode)
        triples to use, in that order (the caller's graph.relations[mode] order); by default the index's relations out of
        `mode` in index order. A pure function of (seed, relation, batch position, the index): min(ceil(len * keep_prob),
        max_keep) entries of every list, the whole list in CSR order where that is all of it, unused slots -1."""
        if relations is None:
            relations = [r for r in self.rels if r[0] == mode]
        relations = [tuple(r) for r in relations]
        for r in relations:
            if r not in self.rel_index or r[0] != mode:
                raise KeyError('KGIndex.sample_neighbours: no adjacency for relation %r out of mode %r' % (r, mode))
        rows = rows.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        R, B, max_keep = len(relations), int(rows.shape[0]), int(max_keep)
        if R < 1:
            raise ValueError('KGIndex.sample_neighbours: mode %r has no relation to sample' % (mode,))
        neigh = torch.empty((R, B, max_keep), dtype=torch.int64, device=self.device)
        counts = torch.empty((R, B), dtype=torch.int32, device=self.device)
        use = np.asarray([self.rel_index[r] for r in relations], dtype=np.int32)
        err = self.err if err is None else err
        with self._call() as (lib, stream):
            _capi.check(lib, lib.mpqe_kg_sample_neighbours(
                self._off_arr, self._rows_arr, self._edges_arr, self.rel_src.ctypes.data, self.rel_dst.ctypes.data,
                len(self.rels), self.mode_rows.ctypes.data, len(self.modes), use.ctypes.data, R, rows.data_ptr() if B else None,
                B, float(keep_prob), max_keep, int(seed) & (2 ** 64 - 1), neigh.data_ptr() if B else None,
                counts.data_ptr() if B else None, err.data_ptr(), stream), 'mpqe_kg_sample_neighbours')
        return relations, neigh, counts

    # ------------------------------------------------------------------------------------------ mixed formulas
    def table(self):
        """The index as one device table (mpqe_kg_table_build), built on first use and kept -> its aligned address."""
        if self._table is None:
            if not self.rels:
                raise ValueError('KGIndex: the index has no relation')
            R, M = len(self.rels), len(self.modes)
            reverse = np.asarray([self.rel_index.get(reverse_relation(r), -1) for r in self.rels], dtype=np.int32)
            valid = (ctypes.c_void_p * M)(*[self.valid[m].data_ptr() for m in self.modes])
            row_ids = (ctypes.c_void_p * M)(*[self.row_ids[m].data_ptr() for m in self.modes])
            with self._call() as (lib, stream):
                need = lib.mpqe_kg_table_bytes(R, M)
                if need == 0:
                    raise ValueError('KGIndex: more relations or modes than the device table covers')
                buf = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
                ptr = _capi._align256(buf.data_ptr())
                _capi.check(lib, lib.mpqe_kg_table_build(self._off_arr, self._rows_arr, self._edges_arr, self.rel_src.ctypes.data,
                                                         self.rel_dst.ctypes.data, reverse.ctypes.data, R,
                                                         self.mode_rows.ctypes.data, valid, row_ids, M, ptr, need, stream),
                            'mpqe_kg_table_build')
            ne = np.asarray([self.num_entities[m] for m in self.modes], dtype=np.int64)
            base = np.zeros(M, dtype=np.int64)
            base[1:] = np.cumsum(self.mode_rows)[:-1]
            self._table = (buf, ptr)
            self._num_entities_host, self._mode_base_host = ne, base
            self._num_entities_dev = torch.from_numpy(ne).to(self.device)
            self._row_ids_cat_host = np.concatenate([self.row_ids_host[m] for m in self.modes])
        return self._table[1]

    def records_of(self, formulas, queries):
        """Records [Q, 10] int64 on the device, in the layout sample_queries writes, of graph.Query objects (or anchor id
        lists) with their formulas: one formula for all of them, or one per query. Only what answers_mixed reads is filled:
        the relation indices, the anchors' rows as the leaf edges' destinations, and edge 0's source row (the target's, -1
        without a Query); every other row is -1. All formulas must be of one query type."""
        formulas = [formulas] * len(queries) if isinstance(formulas, Formula) else list(formulas)
        if len(formulas) != len(queries):
            raise ValueError('KGIndex.records_of: one formula per query')
        out = np.full((len(queries), _capi.KG_QUERY_INTS), -1, dtype=np.int64)
        if formulas and len(set(f.query_type for f in formulas)) != 1:
            raise ValueError('KGIndex.records_of: queries of one query type')
        for i, (f, q) in enumerate(zip(formulas, queries)):
            for e, r in enumerate(_edge_relations(f)):
                if r not in self.rel_index:
                    raise KeyError('KGIndex: no adjacency for relation %r' % (r,))
                out[i, 2 + 3 * e] = self.rel_index[r]
            anchors = q.anchor_nodes if hasattr(q, 'anchor_nodes') else q
            for slot, e in enumerate(QUERY_SHAPES[f.query_type][1]):
                out[i, 3 + 3 * e] = self._rows_of(f.anchor_modes[slot], np.asarray([anchors[slot]], dtype=np.int64))[0]
            if hasattr(q, 'target_node'):
                out[i, 1] = self._rows_of(f.target_mode, np.asarray([q.target_node], dtype=np.int64))[0]
            out[i, 0] = 1
        return torch.from_numpy(out).to(self.device)

    def _rows_of_modes(self, mode_index, ids):
        """_rows_of for ids whose modes differ: mode_index [B] and ids [B] int64 on the device -> table rows [B], computed
        there; an id that is no entity of its mode becomes that mode's row n (outside)."""
        dev = self.device
        if self._maps_dev is None:
            self._maps_dev = torch.from_numpy(self.maps_host).to(dev)
        cat = self.__dict__.get('_row_ids_cat_dev')
        if cat is None:
            base = np.zeros(len(self.modes), dtype=np.int64)
            base[1:] = np.cumsum(self.mode_rows)[:-1]
            cat = self.__dict__['_row_ids_cat_dev'] = (
                torch.cat([self.row_ids[m] for m in self.modes]), torch.from_numpy(base).to(dev),
                torch.from_numpy(self.mode_rows).to(dev))
        row_ids, base, rows = cat
        maps = self._maps_dev
        n = rows[mode_index]
        inside = (ids >= 0) & (ids < maps.shape[0])
        cand = torch.where(inside, maps[ids.clamp(0, maps.shape[0] - 1)], torch.full_like(ids, -1))
        ok = (cand >= 0) & (cand < n)
        ok &= row_ids[base[mode_index] + torch.minimum(cand.clamp(min=0), n - 1)] == ids
        return torch.where(ok, cand, n)

    def records_of_ids(self, formulas, formula_of, anchors, targets=None):
        """records_of for ids that are on the device already (kg.MixedQuerySet windows): formulas a sequence of Formula of
        one query type, formula_of [Q] int64 every query's position in it, anchors [Q, A] and targets [Q] (or None: -1)
        global ids. -> records [Q, 10] int64, equal to records_of(the queries' formulas, the queries), from tensor ops
        alone: a per-formula template (kept per `formulas` object) gathered by formula_of, the anchors' and the target's
        rows through the device copy of node_maps. A formula_of outside the formulas gives a record without a query."""
        dev = self.device
        kept = self.__dict__.setdefault('_record_templates', {})
        hit = kept.get(id(formulas))
        if hit is None or hit[0] is not formulas:
            if len(formulas) == 0 or len({f.query_type for f in formulas}) != 1:
                raise ValueError('KGIndex.records_of_ids: formulas of one query type')
            anchor_edges = list(QUERY_SHAPES[formulas[0].query_type][1])
            tmpl = np.full((len(formulas), _capi.KG_QUERY_INTS), -1, dtype=np.int64)
            modes = np.zeros((len(formulas), len(anchor_edges) + 1), dtype=np.int64)
            for k, f in enumerate(formulas):
                for e, r in enumerate(_edge_relations(f)):
                    if r not in self.rel_index:
                        raise KeyError('KGIndex: no adjacency for relation %r' % (r,))
                    tmpl[k, 2 + 3 * e] = self.rel_index[r]
                tmpl[k, 0] = 1
                modes[k] = [self.mode_index[m] for m in f.anchor_modes] + [self.mode_index[f.target_mode]]
            while len(kept) >= 16:
                kept.pop(next(iter(kept)))
            hit = kept[id(formulas)] = (formulas, torch.from_numpy(tmpl).to(dev), torch.from_numpy(modes).to(dev), anchor_edges)
        _, tmpl, modes, anchor_edges = hit
        fo = formula_of.to(device=dev, dtype=torch.int64).reshape(-1)
        anchors = anchors.to(device=dev, dtype=torch.int64).reshape(fo.shape[0], len(anchor_edges))
        ok = (fo >= 0) & (fo < tmpl.shape[0])
        foc = fo.clamp(0, tmpl.shape[0] - 1)
        rec = tmpl[foc]
        for slot, e in enumerate(anchor_edges):
            rec[:, 3 + 3 * e] = self._rows_of_modes(modes[foc, slot], anchors[:, slot].contiguous())
        if targets is not None:
            rec[:, 1] = self._rows_of_modes(modes[foc, -1], targets.to(device=dev, dtype=torch.int64).reshape(-1))
        return torch.where(ok[:, None], rec, torch.full_like(rec, -1))

    def answers_mixed(self, query_type, records, hard=False, probe_rows=None, bits=True, global_bits=False,
                      max_bitmap_bytes=1 << 30):
        """The exact answers of a batch of queries of one query type whose relations differ per query, one launch (per
        chunk): records [Q, 10] int64 on the device as sample_queries / records_of give them -> KGAnswersMixed. hard: the
        hard negatives' sets and counts too. probe_rows [Q]: the rows whose membership in the answers `member` reports
        (default: the records' target rows). bits=False: counts, target_mode and member only, no bitmap leaves the kernel.
        The bitmaps are [Q, W(widest mode)]; where they -- with the workspace of modes too wide for LDS -- pass
        max_bitmap_bytes, the batch is walked in chunks and the bitmaps are not kept: the sampled CSRs recompute them
        chunk by chunk (the draw key takes the query's position in the whole batch, so the chunking changes nothing)."""
        qt = _capi.QUERY_TYPE_IDS[query_type] if isinstance(query_type, str) else int(query_type)
        records = records.to(device=self.device, dtype=torch.int64).contiguous()
        if probe_rows is not None:
            probe_rows = probe_rows.to(device=self.device, dtype=torch.int64).contiguous()
        out = KGAnswersMixed(self, qt, records, bool(hard), probe_rows, bool(global_bits), int(max_bitmap_bytes))
        out._fill(bool(bits))
        return out

    def _records_by_formula(self, qt_name, records):
        """The accepted slots of a host [Q, 10] array grouped by formula -> {Formula: (slots, target rows [B], anchor rows
        [B, A], variable rows [B, V])}; the same reading of the query tuple as graph.Query's."""
        slots = np.nonzero(records[:, 0] == 1)[0]
        n_edges, anchor_edges, variable_edges, _ = QUERY_SHAPES[qt_name]
        e = records[slots, 1:1 + 3 * n_edges].reshape(-1, n_edges, 3)
        out = {}
        if slots.size == 0:
            return out
        keys, inverse = np.unique(e[:, :, 1], axis=0, return_inverse=True)
        inverse = inverse.reshape(-1)
        for g, rel_ids in enumerate(keys):
            pick = np.nonzero(inverse == g)[0]
            x, y = e[pick, :, 0], e[pick, :, 2]
            out[self._formula_of(qt_name, rel_ids)] = (slots[pick], x[:, 0].copy(), np.ascontiguousarray(y[:, list(anchor_edges)]),
                                                       np.ascontiguousarray(y[:, list(variable_edges)]))
        return out

    def sample_query_sets(self, query_types, per_type, seed, neg_sample_max=100, train_index=None, max_rounds=8,
                          max_tries=8, batched=False):
        """The reference's Graph.sample_queries (train_index None) / sample_test_queries pipeline on the device: walk,
        group the accepted slots by formula, one answers(hard=True) call per formula, keep a query only if it has a
        negative (and, for the intersection types, a hard negative) and -- with train_index, an index of the same modes and
        node map over the training edges -- only if its target does NOT answer it on the training graph; then at most
        neg_sample_max negatives / hard negatives per kept query. Rounds repeat until `per_type` queries per type or
        max_rounds. -> {Formula: QuerySet}. A pure function of (seed, the index).

        batched=True: the same walk, filter and "first `want` accepted slots" rule, and so the same queries per formula in
        the same order, at a cost per query TYPE instead of per formula: per type and round one answers_mixed(hard) call
        over all slots, one member-only call on train_index, the filter as tensor operations, one read-back, one negative
        and one hard draw. The kept queries of a type are ordered by (formula's relation indices ascending, round, slot)
        in one store; every formula's QuerySet is a slice of it with its offsets_host mirror filled.
        Seeds. With type_seed = seed * 1000003 + 7919 * type id (mod 2^63), round r walks with type_seed + 104729 r in both
        forms. The default draws formula number g's negatives (g = 0, 1, ... in ascending relation indices within the
        round) with that + 15485863 (g + 1), the hard negatives with one more, keyed by the query's position among the
        formula's kept queries of the round. batched=True draws the whole round with type_seed + 104729 r + 15485863 (hard:
        one more), keyed by the query's position among ALL the round's kept queries in the store's order; QuerySet.draw
        holds (seed, position) per query. With neg_sample_max at or above every list's length both forms give every
        list whole and ascending, hence the same sets; below it they draw different uniform subsets."""
        if batched:
            return self._sample_query_sets_batched(query_types, int(per_type), seed, int(neg_sample_max), train_index,
                                                   int(max_rounds), max_tries)
        sets = {}
        for qt_name in query_types:
            have, parts = 0, {}
            type_seed = (int(seed) * 1000003 + 7919 * _capi.QUERY_TYPE_IDS[qt_name]) & (2 ** 63 - 1)
            for rnd in range(int(max_rounds)):
                want = int(per_type) - have
                if want <= 0:
                    break
                slots = 2 * want + 64
                records = self.sample_queries(qt_name, slots, type_seed + 104729 * rnd, max_tries).cpu().numpy()
                groups = self._records_by_formula(qt_name, records)
                kept = {}
                for formula, (where, target, anchors, variables) in groups.items():
                    prog, order = self.programme(formula)
                    rows = torch.from_numpy(np.ascontiguousarray(anchors[:, order].T)).to(self.device)
                    ans = self.answers_of_rows(formula, prog, rows, hard=True)
                    ok = ans.counts[0] < self.num_entities[formula.target_mode]
                    if 'inter' in qt_name:
                        ok &= ans.counts[1] > 0
                    t = torch.from_numpy(target).to(self.device)
                    if train_index is not None:
                        t_prog, _ = train_index.programme(formula)
                        seen = train_index.answers_of_rows(formula, t_prog, rows).bits
                        ok &= ((seen.gather(1, (t >> 5).unsqueeze(1)).squeeze(1) >> (t & 31)) & 1) == 0
                    kept[formula] = (ans, ok.cpu().numpy())
                accepted = np.sort(np.concatenate([groups[f][0][kept[f][1]] for f in groups] or [np.zeros(0, np.int64)]))
                last = accepted[want - 1] if accepted.size >= want else slots
                for k, formula in enumerate(groups):
                    where, target, anchors, variables = groups[formula]
                    ans, ok = kept[formula]
                    pick = np.nonzero(ok & (where <= last))[0]
                    if pick.size == 0:
                        continue
                    sub = ans.subset(torch.from_numpy(pick).to(self.device))
                    draw = type_seed + 104729 * rnd + 15485863 * (k + 1)
                    neg = sub.sample_negative_csr(neg_sample_max, draw)
                    hard = sub.sample_hard_csr(neg_sample_max, draw + 1) if 'inter' in qt_name else None
                    parts.setdefault(formula, []).append((target[pick], anchors[pick], variables[pick], neg, hard))
                    have += pick.size
            for formula, chunks in parts.items():
                sets[formula] = QuerySet._from_parts(self, formula, chunks)
        return sets

    def _formula_of(self, qt_name, rel_ids):
        rels = [self.rels[int(r)] for r in rel_ids]
        return Formula(qt_name, (rels[0], (rels[1], rels[2])) if QUERY_SHAPES[qt_name][3] else tuple(rels))

    def _sample_query_sets_batched(self, query_types, per_type, seed, k, train_index, max_rounds, max_tries):
        dev = self.device
        self.table()
        remap = None
        if train_index is not None:
            # a relation's index in the training index; -1 where that index cannot walk it (it lacks the relation itself --
            # the record names it -- or its inverse, whose CSR the hop walks)
            remap_host = np.asarray([train_index.rel_index[r] if r in train_index.rel_index and
                                     reverse_relation(r) in train_index.rel_index else -1 for r in self.rels], dtype=np.int64)
            remap = torch.from_numpy(remap_host).to(dev)
        sets = {}
        clock = [time.perf_counter()]

        def tick(section):
            if self.section_times is not None:
                if dev.type == 'cuda':
                    torch.cuda.synchronize(dev)
                now = time.perf_counter()
                self.section_times[section] = self.section_times.get(section, 0.0) + now - clock[0]
                clock[0] = now
        for qt_name in query_types:
            n_e, anchor_edges, variable_edges, _ = QUERY_SHAPES[qt_name]
            a_cols, v_cols, inter = list(anchor_edges), list(variable_edges), 'inter' in qt_name
            rel_cols = slice(2, 2 + 3 * n_e, 3)
            have, parts = 0, []
            type_seed = (int(seed) * 1000003 + 7919 * _capi.QUERY_TYPE_IDS[qt_name]) & (2 ** 63 - 1)
            for rnd in range(max_rounds):
                want = per_type - have
                if want <= 0:
                    break
                slots = 2 * want + 64
                round_seed = type_seed + 104729 * rnd
                records = self.sample_queries(qt_name, slots, round_seed, max_tries)
                tick('walk')
                ans = self.answers_mixed(qt_name, records, hard=inter)
                tick('answers')
                found = records[:, 0] == 1
                ok = found & (ans.target_mode >= 0) & (ans.negative_counts() > 0)
                if inter:
                    ok &= ans.counts[1] > 0
                missing = torch.zeros_like(ok)
                if train_index is not None:
                    named = records[:, rel_cols]
                    mapped = torch.where(named >= 0, remap[named.clamp(min=0)], torch.full_like(named, -1))
                    missing = found & (mapped < 0).any(dim=1)
                    on_train = records.clone()
                    on_train[:, rel_cols] = mapped
                    on_train[:, 0] = torch.where(missing, torch.zeros_like(records[:, 0]), records[:, 0])
                    ok &= train_index.answers_mixed(qt_name, on_train, bits=False).member == 0
                    tick('train filter')
                host = torch.cat([records, ok.long().unsqueeze(1), missing.long().unsqueeze(1), ans.counts.t(),
                                  ans.target_mode.long().unsqueeze(1)], dim=1).cpu().numpy()      # the round's one read-back
                tick('filter + read-back')
                rec, ok_h, missing_h = host[:, :_capi.KG_QUERY_INTS], host[:, 10] != 0, host[:, 11] != 0
                if missing_h.any():
                    for r in rec[np.nonzero(missing_h)[0][0], rel_cols]:
                        for rel in (reverse_relation(self.rels[int(r)]), self.rels[int(r)]):
                            if rel not in train_index.rel_index:
                                raise KeyError('KGIndex: no adjacency for relation %r' % (rel,))
                accepted = np.nonzero(ok_h)[0]
                last = accepted[want - 1] if accepted.size >= want else slots
                keep = accepted[accepted <= last]
                if keep.size == 0:
                    continue
                rel = rec[keep][:, rel_cols]
                keep = keep[np.lexsort(tuple(rel[:, c] for c in reversed(range(n_e))))]       # (stable: slots ascending)
                K = keep.size
                rec_k, c0, c1, mode = rec[keep], host[keep, 12], host[keep, 13], host[keep, 14]
                sub = ans.subset(torch.from_numpy(keep).to(dev))
                tick('host pick + subset')

                def scan(lengths):
                    off = np.zeros(K + 1, dtype=np.int64)
                    np.cumsum(np.minimum(lengths, k), out=off[1:])
                    return off
                neg_off = scan(self._num_entities_host[mode] - c0)
                hard_off = scan(c1) if inter else None
                drawn = sub._sample_many([(0, k, round_seed + 15485863, neg_off)] +
                                         ([(1, k, round_seed + 15485864, hard_off)] if inter else []))
                neg, hard = drawn[0][0], drawn[1][0] if inter else None
                tick('draws')
                e = rec_k[:, 1:1 + 3 * n_e].reshape(K, n_e, 3)
                src_ids = self._row_ids_cat_host[self._mode_base_host[self.rel_src[e[:, :, 1]]] + e[:, :, 0]]
                dst_ids = self._row_ids_cat_host[self._mode_base_host[self.rel_dst[e[:, :, 1]]] + e[:, :, 2]]
                parts.append(dict(rel=e[:, :, 1], rnd=np.full(K, rnd), slot=keep, targets=src_ids[:, 0], anchors=dst_ids[:, a_cols],
                                  variables=dst_ids[:, v_cols], neg=neg, neg_off=neg_off, hard=hard, hard_off=hard_off,
                                  seed=np.full(K, round_seed + 15485863), pos=np.arange(K)))
                have += K
            if parts:
                self._store_sets(qt_name, parts, sets)
            tick('ids + sets')
        return sets

    def _store_sets(self, qt_name, parts, sets):
        """the rounds' kept queries as ONE store ordered by (relation indices, round, slot), and its slices per formula"""
        dev = self.device
        cat = lambda key: np.concatenate([p[key] for p in parts])                       # noqa: E731
        rel = cat('rel')
        n_e = rel.shape[1]
        perm = None
        if len(parts) > 1:
            perm = np.lexsort((cat('slot'), cat('rnd')) + tuple(rel[:, c] for c in reversed(range(n_e))))
            rel = rel[perm]

        def csr(ids_key, off_key):
            if parts[0][ids_key] is None:
                return None, None
            ids = torch.cat([p[ids_key] for p in parts])
            lens = np.concatenate([np.diff(p[off_key]) for p in parts])
            starts = np.zeros(lens.size + 1, dtype=np.int64)
            np.cumsum(lens, out=starts[1:])
            if perm is None:
                return (ids, torch.from_numpy(starts).to(dev)), starts
            off = np.zeros(lens.size + 1, dtype=np.int64)
            np.cumsum(lens[perm], out=off[1:])
            take = np.repeat(starts[:-1][perm] - off[:-1], lens[perm]) + np.arange(int(off[-1]))
            return (ids[torch.from_numpy(take).to(dev)], torch.from_numpy(off).to(dev)), off

        def ids(key):
            a = cat(key)
            return torch.from_numpy(np.ascontiguousarray(a if perm is None else a[perm])).to(dev)
        neg, neg_off = csr('neg', 'neg_off')
        hard, hard_off = csr('hard', 'hard_off')
        targets, anchors, variables = ids('targets'), ids('anchors'), ids('variables')
        seeds, pos = cat('seed'), cat('pos')
        if perm is not None:
            seeds, pos = seeds[perm], pos[perm]
        keys, first = np.unique(rel, axis=0, return_index=True)
        bounds = [int(b) for b in first] + [int(rel.shape[0])]
        G = len(keys)

        def rebased(off):
            """every formula's own offsets (from 0), end to end: one upload; a formula's are a view of it"""
            if off is None:
                return None, None
            host = [off[bounds[g]:bounds[g + 1] + 1] - off[bounds[g]] for g in range(G)]
            return host, torch.from_numpy(np.concatenate(host)).to(dev)
        neg_host, neg_dev = rebased(neg_off)
        hard_host, hard_dev = rebased(hard_off)
        for g, rel_ids in enumerate(keys):
            lo, hi = bounds[g], bounds[g + 1]

            def cut(pair, off, dev_off):
                if pair is None:
                    return None
                return pair[0][int(off[lo]):int(off[hi])], dev_off[lo + g:hi + g + 1]
            qs = QuerySet(self, self._formula_of(qt_name, rel_ids), targets[lo:hi], anchors[lo:hi], variables[lo:hi],
                          cut(neg, neg_off, neg_dev), cut(hard, hard_off, hard_dev))
            qs.__dict__['_offsets_host'] = {False: neg_host[g], True: None if hard_host is None else hard_host[g]}
            qs.draw = (seeds[lo:hi], pos[lo:hi])
            sets[qs.formula] = qs

class KGAnswers(object):
    """What KGIndex.answers returns. On the device: bits [Q, W] (the answers), hard_bits [Q, W] or None, counts [2, Q]
    int64 (|answers|, |hard|); int32 tensors holding the uint32 words. Rows are table rows of `mode` (n of them)."""

    def __init__(self, index, formula, mode, n, bits, hard_bits, counts):
        self.index, self.formula, self.mode, self.n = index, formula, mode, n
        self.bits, self.hard_bits, self.counts = bits, hard_bits, counts

    def __len__(self):
        return int(self.bits.shape[0])

    def _compact(self, bits, select, lengths):
        """(offsets [Q + 1], rows) int64 on the device: mpqe_kg_rows"""
        Q = len(self)
        dev = self.index.device
        offsets = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
        if Q == 0:
            return offsets, torch.zeros(0, dtype=torch.int64, device=dev)
        torch.cumsum(lengths, 0, out=offsets[1:])
        total = int(offsets[-1].item())
        rows = torch.empty(total, dtype=torch.int64, device=dev)
        with self.index._call() as (lib, stream):
            _capi.check(lib, lib.mpqe_kg_rows(bits.data_ptr(), Q, self.n, self.index.valid[self.mode].data_ptr(), select,
                                              offsets.data_ptr(), rows.data_ptr() if total else None, total,
                                              self.index.err.data_ptr(), stream), 'mpqe_kg_rows')
        return offsets, rows

    def subset(self, pick):
        """the answers of the queries `pick` (a device index tensor) alone"""
        return KGAnswers(self.index, self.formula, self.mode, self.n, self.bits[pick].contiguous(),
                         None if self.hard_bits is None else self.hard_bits[pick].contiguous(),
                         self.counts[:, pick].contiguous())

    def _sample_ids_csr(self, bits, select, lengths, k, seed):
        """(ids, offsets) on the device: mpqe_kg_sample_rows -- at most k members of every query's set"""
        Q = len(self)
        dev = self.index.device
        k = int(k)
        offsets = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
        if Q == 0:
            return torch.zeros(0, dtype=torch.int64, device=dev), offsets
        torch.cumsum(torch.clamp(lengths, max=k), 0, out=offsets[1:])
        total = int(offsets[-1].item())
        rows = torch.empty(total, dtype=torch.int64, device=dev)
        with self.index._call() as (lib, stream):
            _capi.check(lib, lib.mpqe_kg_sample_rows(bits.data_ptr(), Q, self.n, self.index.valid[self.mode].data_ptr(),
                                                     select, offsets.data_ptr(), rows.data_ptr() if total else None, total,
                                                     k, int(seed) & (2 ** 64 - 1), self.index.err.data_ptr(), stream),
                        'mpqe_kg_sample_rows')
        return self.index.row_ids[self.mode][rows], offsets

    def sample_negative_csr(self, k, seed):
        """negative_csr() with at most k ids a query (the reference's Query(neg_sample_max), graph.py:83-87): all of them
        ascending where there are at most k, otherwise k distinct ones, a uniform subset, a pure function of (seed, the
        query's position, its set). Q x k ids at most, where negative_csr() is Q x (entities of the mode)."""
        return self._sample_ids_csr(self.bits, _capi.KG_ROWS_COMPLEMENT,
                                    self.index.num_entities[self.mode] - self.counts[0], k, seed)

    def sample_hard_csr(self, k, seed):
        if self.hard_bits is None:
            raise ValueError('KGAnswers: computed without hard=True')
        return self._sample_ids_csr(self.hard_bits, _capi.KG_ROWS_SET, self.counts[1], k, seed)

    def exclusion_csr(self):
        """(offsets, rows): per query its answers and the rows below n that are no entity, ascending -- what
        ops.rank_entities takes as `exclude` for the filtered setting."""
        holes = self.n - self.index.num_entities[self.mode]
        return self._compact(self.bits, _capi.KG_ROWS_WITH_HOLES, self.counts[0] + holes)

    def _ids_csr(self, bits, select, lengths):
        offsets, rows = self._compact(bits, select, lengths)
        return self.index.row_ids[self.mode][rows], offsets

    def answer_csr(self):
        """(ids, offsets): the answers as global entity ids, CSR on the device"""
        return self._ids_csr(self.bits, _capi.KG_ROWS_SET, self.counts[0])

    def negative_csr(self):
        """(ids, offsets): every entity of the mode that is no answer (full_sets[mode] - answers), the form
        NegativeSampler.from_csr takes"""
        return self._ids_csr(self.bits, _capi.KG_ROWS_COMPLEMENT, self.index.num_entities[self.mode] - self.counts[0])

    def hard_csr(self):
        if self.hard_bits is None:
            raise ValueError('KGAnswers: computed without hard=True')
        return self._ids_csr(self.hard_bits, _capi.KG_ROWS_SET, self.counts[1])

    def _lists(self, words):
        row_ids = self.index.row_ids_host[self.mode]
        return [row_ids[r] for r in _unpack(words.cpu().numpy(), self.n)]

    def lists(self):
        """per query the answers as global entity ids (host arrays; for tests and small uses)"""
        return self._lists(self.bits)

    def hard_lists(self):
        if self.hard_bits is None:
            raise ValueError('KGAnswers: computed without hard=True')
        return self._lists(self.hard_bits)

    def negative_lists(self):
        valid = self.index.valid[self.mode]
        return self._lists(valid.unsqueeze(0) & ~self.bits)

    def check(self):
        self.index.check()


class KGAnswersMixed(object):
    """What KGIndex.answers_mixed returns, on the device: counts [2, Q] int64 (|answers|, |hard|; the latter 0 without
    hard=True), target_mode [Q] int32 (mode INDEX, -1 for a record without a query and for a malformed one), member [Q] int32
    (is the probe row an answer), and -- when asked for and within max_bitmap_bytes -- bits / hard_bits [Q, W(widest mode)]
    int32 holding uint32 words (None otherwise: recomputed per chunk where needed)."""

    def __init__(self, index, qt, records, hard, probe_rows, global_bits, max_bitmap_bytes):
        self.index, self.qt, self.records, self.hard, self.probe_rows = index, qt, records, hard, probe_rows
        self.global_bits, self.max_bitmap_bytes = global_bits, max_bitmap_bytes
        self.W = _words(int(index.mode_rows.max()))
        self.bits = self.hard_bits = None
        Q, dev = len(self), index.device
        self.counts = torch.zeros((2, Q), dtype=torch.int64, device=dev)
        self.target_mode = torch.full((Q,), -1, dtype=torch.int32, device=dev)
        self.member = torch.zeros((Q,), dtype=torch.int32, device=dev)

    def __len__(self):
        return int(self.records.shape[0])

    def _flags(self):
        return (_capi.KG_GLOBAL_BITS if self.global_bits else 0) | (_capi.KG_COUNT_HARD if self.hard else 0)

    def _chunk(self, with_bits):
        """queries a launch: the bitmaps that leave it and, for modes too wide for LDS, its workspace within the budget"""
        index = self.index
        with index._call() as (lib, _):
            one = lib.mpqe_kg_mixed_workspace_bytes(1, index.mode_rows.ctypes.data, len(index.modes), self._flags())
        if one == 0:
            raise ValueError('KGIndex.answers_mixed: modes outside what the kernel covers')
        per = (16 * self.W if one > 256 else 0) + (4 * self.W * (2 if self.hard else 1) if with_bits else 0)
        return max(1, min(len(self), self.max_bitmap_bytes // per)) if per else max(1, len(self))

    def _run(self, lo, hi, with_bits, results):
        """one launch over the queries [lo, hi) -> (bits, hard_bits) or (None, None); results: also fill counts etc."""
        index, dev, n = self.index, self.index.device, hi - lo
        bits = torch.empty((n, self.W), dtype=torch.int32, device=dev) if with_bits else None
        hard_bits = torch.empty((n, self.W), dtype=torch.int32, device=dev) if with_bits and self.hard else None
        counts = torch.empty((2, n), dtype=torch.int64, device=dev) if results else None
        target = torch.empty((n,), dtype=torch.int32, device=dev)
        member = torch.empty((n,), dtype=torch.int32, device=dev) if results else None
        table = index.table()
        with index._call() as (lib, stream):
            need = lib.mpqe_kg_mixed_workspace_bytes(n, index.mode_rows.ctypes.data, len(index.modes), self._flags())
            ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
            _capi.check(lib, lib.mpqe_kg_answers_mixed(
                table, index.mode_rows.ctypes.data, len(index.modes), self.qt, self.records[lo:hi].data_ptr(), n,
                None if self.probe_rows is None else self.probe_rows[lo:hi].data_ptr(), ops._p(bits), ops._p(hard_bits),
                self.W, ops._p(counts), target.data_ptr(), ops._p(member), self._flags(), _capi._align256(ws.data_ptr()), need,
                index.err.data_ptr(), stream), 'mpqe_kg_answers_mixed')
        if results:
            self.counts[:, lo:hi], self.target_mode[lo:hi], self.member[lo:hi] = counts, target, member
        return bits, hard_bits

    def _fill(self, want_bits):
        Q = len(self)
        if Q == 0:
            return
        keep = want_bits and self._chunk(True) >= Q
        step = self._chunk(keep)
        for lo in range(0, Q, step):
            got = self._run(lo, min(Q, lo + step), keep, True)
            if keep:
                self.bits, self.hard_bits = got         # (keep: one chunk holds the whole batch)

    def _bit_chunks(self):
        """(lo, hi, bits, hard_bits) over the batch: the kept bitmaps, or each chunk's recomputed"""
        Q = len(self)
        if self.bits is not None or Q == 0:
            if Q:
                yield 0, Q, self.bits, self.hard_bits
            return
        step = self._chunk(True)
        for lo in range(0, Q, step):
            hi = min(Q, lo + step)
            yield (lo, hi) + self._run(lo, hi, True, False)

    def subset(self, pick):
        """the answers of the queries `pick` (a device index tensor) alone, in that order"""
        out = KGAnswersMixed(self.index, self.qt, self.records[pick].contiguous(), self.hard,
                             None if self.probe_rows is None else self.probe_rows[pick].contiguous(), self.global_bits,
                             self.max_bitmap_bytes)
        out.counts, out.target_mode, out.member = self.counts[:, pick].contiguous(), self.target_mode[pick].contiguous(), \
            self.member[pick].contiguous()
        if self.bits is not None:
            out.bits = self.bits[pick].contiguous()
            out.hard_bits = None if self.hard_bits is None else self.hard_bits[pick].contiguous()
        return out

    def negative_counts(self):
        """[Q] int64: entities of the query's target mode that are no answer (0 for a query that produced nothing)"""
        self.index.table()
        mode = self.target_mode.long()
        full = self.index._num_entities_dev[mode.clamp(min=0)]
        return torch.where(mode >= 0, full - self.counts[0], torch.zeros_like(full))

    def _sample_many(self, draws):
        """draws: [(0 answers' complement | 1 hard set, k, seed, offsets_host or None)] -> [(ids, offsets)] on the device:
        mpqe_kg_sample_rows_mixed per chunk of bitmaps and draw, q_base = the chunk's first query. The bitmaps that were
        not kept are recomputed ONCE per chunk for all the draws. offsets_host: the exclusive scan of min(length, k) where
        the caller has it already (no read-back then)."""
        index, dev, Q = self.index, self.index.device, len(self)
        plans = []
        for which, k, seed, offsets_host in draws:
            if which and not self.hard:
                raise ValueError('KGAnswersMixed: computed without hard=True')
            k = int(k)
            if offsets_host is not None:
                offsets = torch.from_numpy(np.ascontiguousarray(offsets_host, dtype=np.int64)).to(dev)
                total = int(offsets_host[-1])
            else:
                offsets = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
                if Q:
                    torch.cumsum(torch.clamp(self.counts[1] if which else self.negative_counts(), max=k), 0, out=offsets[1:])
                total = int(offsets[-1].item()) if Q else 0
            plans.append((which, k, int(seed) & (2 ** 64 - 1), offsets, total, torch.empty(total, dtype=torch.int64, device=dev)))
        if Q:
            table = index.table()
            for lo, hi, bits, hard_bits in self._bit_chunks():
                for which, k, seed, offsets, total, ids in plans:
                    with index._call() as (lib, stream):
                        _capi.check(lib, lib.mpqe_kg_sample_rows_mixed(
                            table, index.mode_rows.ctypes.data, len(index.modes), (hard_bits if which else bits).data_ptr(),
                            self.W, self.target_mode[lo:hi].data_ptr(), hi - lo, lo,
                            _capi.KG_ROWS_SET if which else _capi.KG_ROWS_COMPLEMENT, offsets[lo:].data_ptr(), None,
                            ids.data_ptr() if total else None, total, k, seed, index.err.data_ptr(), stream),
                            'mpqe_kg_sample_rows_mixed')
        return [(p[5], p[3]) for p in plans]

    def sample_negative_csr(self, k, seed, offsets_host=None):
        """(ids, offsets): per query at most k entities of its target mode that are no answer -- KGAnswers.sample_negative_csr
        with the mode taken per query; the draw of query q is keyed by (seed, q), q its position in this batch."""
        return self._sample_many([(0, k, seed, offsets_host)])[0]

    def sample_hard_csr(self, k, seed, offsets_host=None):
        return self._sample_many([(1, k, seed, offsets_host)])[0]

    def _lists(self, which):
        index, out = self.index, []
        for lo, hi, bits, hard_bits in self._bit_chunks():
            words = (hard_bits if which else bits).cpu().numpy()
            modes = self.target_mode[lo:hi].cpu().numpy()
            for w, m in zip(words, modes):
                if m < 0:
                    out.append(np.zeros(0, dtype=np.int64))
                else:
                    name = index.modes[int(m)]
                    out.append(index.row_ids_host[name][_unpack(w[None, :], int(index.mode_rows[int(m)]))[0]])
        return out

    def lists(self):
        """per query the answers as global entity ids (host arrays; for tests and small uses)"""
        return self._lists(0)

    def hard_lists(self):
        if not self.hard:
            raise ValueError('KGAnswersMixed: computed without hard=True')
        return self._lists(1)

    def check(self):
        self.index.check()


class QuerySet(object):
    """Grounded queries of one formula with their sampled negatives, on the device (KGIndex.sample_query_sets): targets [B],
    anchors [B, A] and variables [B, V] as global entity ids, neg / hard = (ids, offsets [B + 1]) in the form
    NegativeSampler.from_csr takes (hard None for the chain types)."""

    def __init__(self, index, formula, targets, anchors, variables, neg, hard):
        self.index, self.formula = index, formula
        self.targets, self.anchors, self.variables, self.neg, self.hard = targets, anchors, variables, neg, hard

    @classmethod
    def _from_parts(cls, index, formula, chunks):
        dev = index.device

        def ids(mode_of_column, rows):
            cols = [index.row_ids[m][torch.from_numpy(np.ascontiguousarray(rows[:, c])).to(dev)]
                    for c, m in enumerate(mode_of_column)]
            return torch.stack(cols, dim=1) if cols else torch.zeros((rows.shape[0], 0), dtype=torch.int64, device=dev)

        def csr(pairs):
            offsets, base = [torch.zeros(1, dtype=torch.int64, device=dev)], 0
            for _, off in pairs:
                offsets.append(off[1:] + base)
                base += int(off[-1].item())
            return torch.cat([p[0] for p in pairs]), torch.cat(offsets)
        rels = _edge_relations(formula)
        var_modes = [rels[e][2] for e in QUERY_SHAPES[formula.query_type][2]]        # a variable is its edge's y
        target = np.concatenate([c[0] for c in chunks])
        anchors = np.concatenate([c[1] for c in chunks])
        variables = np.concatenate([c[2] for c in chunks])
        return cls(index, formula, ids([formula.target_mode], target[:, None])[:, 0], ids(formula.anchor_modes, anchors),
                   ids(var_modes, variables), csr([c[3] for c in chunks]),
                   None if chunks[0][4] is None else csr([c[4] for c in chunks]))

    def __len__(self):
        return int(self.targets.shape[0])

    def offsets_host(self, hard=False):
        """The host mirror of the negatives' (hard: the hard negatives') offsets, int64 [B + 1]: lengths only, copied once.
        It sizes a window's buffers without a synchronisation (evaluation.eval_*_queries)."""
        mirror = self.__dict__.setdefault('_offsets_host', {})
        if hard not in mirror:
            pair = self.hard if hard else self.neg
            mirror[hard] = None if pair is None else pair[1].cpu().numpy()
        return mirror[hard]

    def __getitem__(self, window):
        """The queries [lo, hi) of a slice (step 1) as a QuerySet of views: the id tensors are slices of this set's, the
        CSRs' offsets are re-based to start at 0. Nothing is copied to the host beyond offsets_host()."""
        if not isinstance(window, slice) or window.step not in (None, 1):
            raise TypeError('QuerySet[...]: a slice with step 1')
        lo, hi, _ = window.indices(len(self))
        hi = max(hi, lo)
        mirror = {}

        def cut(pair, hard):
            if pair is None:
                mirror[hard] = None
                return None
            host = self.offsets_host(hard)
            a, b = int(host[lo]), int(host[hi])
            mirror[hard] = host[lo:hi + 1] - a
            return pair[0][a:b], pair[1][lo:hi + 1] - a
        out = QuerySet(self.index, self.formula, self.targets[lo:hi], self.anchors[lo:hi], self.variables[lo:hi],
                       cut(self.neg, False), cut(self.hard, True))
        out.__dict__['_offsets_host'] = mirror
        return out

    def negative_sampler(self):
        """NegativeSampler over the sampled lists; a 1-chain draws from the whole mode as the reference does (model.py:473)"""
        from .sampling import NegativeSampler
        full = None
        if self.formula.query_type == '1-chain':
            ids = self.index.row_ids_host[self.formula.target_mode]
            full = ids[ids >= 0]
        return NegativeSampler.from_csr(self.neg, self.hard, self.index.device, full_list=full)

    def queries(self):
        """graph.Query objects (host lists; for small sets: the drop-in loop and evaluation.eval_* take these)"""
        from .synthetic import query_graph_tuple
        t, a, v = self.targets.cpu().tolist(), self.anchors.cpu().tolist(), self.variables.cpu().tolist()
        neg, neg_off = self.neg[0].cpu().tolist(), self.neg[1].cpu().tolist()
        hard, hard_off = (None, None) if self.hard is None else (self.hard[0].cpu().tolist(), self.hard[1].cpu().tolist())
        return [Query(query_graph_tuple(self.formula, t[i], a[i], v[i]), neg[neg_off[i]:neg_off[i + 1]],
                      None if hard is None else hard[hard_off[i]:hard_off[i + 1]], keep_graph=True) for i in range(len(t))]


class MixedQuerySet(object):
    """The QuerySets of ONE query type concatenated in their dict's order (evaluation.eval_*_queries over queries of
    different formulas at once; QueryEncoderDecoder.score_ids_mixed): formulas (a tuple of Formula), formula_of [Q] int64
    every query's position in it, targets [Q], anchors [Q, A], neg / hard = (ids, offsets [Q + 1]) CSR over the whole
    (hard None for the chain types) -- all on the device --, and on the host the mirrors that size a window without a
    synchronisation: formula_of_host [Q], bounds [F + 1] (formula f's queries are [bounds[f], bounds[f + 1])) and
    offsets_host()."""

    def __init__(self, index, query_type, formulas, formula_of, targets, anchors, neg, hard, bounds, formula_of_host,
                 offsets_host):
        self.index, self.query_type, self.formulas = index, query_type, tuple(formulas)
        self.formula_of, self.targets, self.anchors, self.neg, self.hard = formula_of, targets, anchors, neg, hard
        self.bounds, self.formula_of_host = bounds, formula_of_host
        self._offsets_host = offsets_host

    def __len__(self):
        return int(self.targets.shape[0])

    def offsets_host(self, hard=False):
        """the host mirror of the negatives' (hard: the hard negatives') offsets, int64 [Q + 1], or None"""
        return self._offsets_host[bool(hard)]

    def negative_sampler(self):
        """NegativeSampler over the concatenation's sampled lists (sampler.sample(positions, seed, hard_negatives)). Unlike
        QuerySet.negative_sampler() a mixed 1-chain window draws from each query's SAMPLED negatives, not from the whole
        target mode: the target modes differ from query to query here, so there is no one list to share."""
        from .sampling import NegativeSampler
        if self.neg is None:
            raise ValueError('MixedQuerySet.negative_sampler: the sets hold no sampled negatives')
        return NegativeSampler.from_csr(self.neg, self.hard, self.index.device)

    def take(self, idx):
        """(formula_of, anchors, targets) of the positions idx (int64 on the device), by tensor indexing: no host work per
        query. Sorted positions put equal formulas next to each other (the set is concatenated by formula): longer
        stretches for the mixed kernels."""
        if not torch.is_tensor(idx) or idx.dtype != torch.long or idx.dim() != 1:
            raise TypeError('MixedQuerySet.take: idx must be an int64 vector')
        idx = idx.to(self.formula_of.device)
        return self.formula_of[idx], self.anchors[idx], self.targets[idx]

    @classmethod
    def from_sets(cls, sets):
        """{Formula: QuerySet} -> {query type: MixedQuerySet}, types and formulas in the dict's order. Tensor concatenations
        and the sets' own host mirrors of their offsets (QuerySet.offsets_host: lengths only, copied once per set): no
        per-query host work, no id on the host."""
        by_type = {}
        for formula, qs in sets.items():
            if not isinstance(qs, QuerySet) or qs.formula != formula:
                raise TypeError('MixedQuerySet.from_sets: {formula: kg.QuerySet of that formula}')
            by_type.setdefault(formula.query_type, []).append(qs)
        out = {}
        for qt, group in by_type.items():
            index, dev = group[0].index, group[0].index.device
            lens = np.array([len(qs) for qs in group], dtype=np.int64)
            bounds = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            fo_host = np.repeat(np.arange(len(group), dtype=np.int64), lens)

            def csr(hard):
                pairs = [qs.hard if hard else qs.neg for qs in group]
                if any(p is None for p in pairs):
                    return None, None
                hosts = [qs.offsets_host(hard) for qs in group]
                base = np.concatenate([[0], np.cumsum([int(h[-1]) for h in hosts])]).astype(np.int64)
                host = np.concatenate([np.zeros(1, dtype=np.int64)] + [h[1:] + base[k] for k, h in enumerate(hosts)])
                offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev)] +
                                    [p[1][1:] + int(base[k]) for k, p in enumerate(pairs)])
                return (torch.cat([p[0] for p in pairs]), offsets), host
            neg, neg_host = csr(False)
            hard, hard_host = csr(True)
            out[qt] = cls(index, qt, [qs.formula for qs in group], torch.from_numpy(fo_host).to(dev),
                          torch.cat([qs.targets for qs in group]), torch.cat([qs.anchors for qs in group]), neg, hard, bounds,
                          fo_host, {False: neg_host, True: hard_host})
        return out
