"""TEST INFRASTRUCTURE ONLY, run where a checkout of the reference exists -- generates tests/golden/kg_sets_small.npz by
IMPORTING the reference's Graph and calling Graph.get_negative_samples / Graph.get_metapath_neighs on a tiny synthetic KG
(directly, not through Query, whose cap samples the lists). Only inputs and recorded sets are written.

    MPQE_REFERENCE=<checkout of the reference> python tools/gen_kg_golden.py

The fixture: the schema (JSON), the adjacency as arrays (adj_rel = index into schema.typed_relations(), adj_src, adj_dst),
and per case the query type, its grounded edges [3, 3] = (node, relation index, node) depth first (-1 padded), the sorted
negatives / hard negatives the reference returned as CSR (neg_off / neg_ids, hard_off / hard_ids), none[c] = 1 where it
returned (None, None) -- an empty negative or hard set -- and for the chain types the sorted get_metapath_neighs set
(meta_off / meta_ids). Twelve grounded queries (two per multi-edge type), six with random anchors, and one 2-inter with
the same edge twice (no hard negative: the reference's (None, None)).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get('MPQE_REFERENCE', '')
OUT = os.path.join(ROOT, 'tests', 'golden', 'kg_sets_small.npz')

QUERY_TYPES = ['2-chain', '3-chain', '2-inter', '3-inter', '3-inter_chain', '3-chain_inter']
SEED, DEGREE = 11, 2


def _flat_edges(query_graph):
    out = []

    def walk(item):
        if len(item) == 3 and not isinstance(item[0], (tuple, list)):
            out.append(item)
        else:
            for sub in item:
                walk(sub)
    walk(query_graph[1:])
    return out


def _csr(sets):
    off = np.zeros(len(sets) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in sets])
    ids = np.array([x for s in sets for x in sorted(s)], dtype=np.int64)
    return off, ids


def main():
    if not os.path.isdir(os.path.join(REF, 'mpqe')):
        raise SystemExit('set MPQE_REFERENCE to a checkout of the reference (found none at %r)' % REF)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, REF)
    import mpqe.graph as rgraph
    from mpqe_amd import synthetic
    schema = synthetic.make_schema(*synthetic.KG_SHAPES['tiny'], seed=SEED)
    adj = synthetic.make_adjacency(schema, degree=DEGREE, seed=SEED)
    typed = schema.typed_relations()
    rel_index = {r: i for i, r in enumerate(typed)}
    graph = rgraph.Graph(None, {m: 1 for m in schema.modes}, schema.relations,
                         {r: {n: set(s) for n, s in adj[r].items()} for r in adj})
    rng = np.random.RandomState(500 + SEED)
    cases = []
    for qt in QUERY_TYPES:
        for grounded in (True, True, False):
            formula = synthetic.sample_formula(schema, qt, rng)
            if grounded:
                q = synthetic.sample_grounded_queries(schema, adj, formula, 1, rng)[0]
            else:
                q = synthetic.sample_queries(schema, formula, 1, rng)[0]
            cases.append((qt, q.query_graph))
    # one 2-inter whose two edges are the same edge: union = intersection, so the reference answers (None, None)
    r = typed[0]
    t = int(schema.ids[r[0]][0])
    a = sorted(adj[r][t])[0]
    cases.append(('2-inter', ('2-inter', (t, r, a), (t, r, a))))
    types, edges, none, neg, hard, meta = [], [], [], [], [], []
    for qt, qg in cases:
        got = graph.get_negative_samples(qg)
        none.append(int(got[0] is None))
        neg.append(set() if got[0] is None else set(got[0]))
        hard.append(set() if got[1] is None else set(got[1]))
        flat = _flat_edges(qg)
        e = np.full((3, 3), -1, dtype=np.int64)
        for i, (x, rel, y) in enumerate(flat):
            e[i] = (x, rel_index[tuple(rel)], y)
        edges.append(e)
        types.append(QUERY_TYPES.index(qt))
        if qt.endswith('-chain'):
            rels = tuple(rgraph._reverse_relation(ed[1]) for ed in qg[1:][::-1])
            meta.append(set(graph.get_metapath_neighs(qg[-1][-1], rels)))
        else:
            meta.append(set())
    src, dst, rel = [], [], []
    for r in typed:
        for n in sorted(adj[r]):
            for d in sorted(adj[r][n]):
                rel.append(rel_index[r])
                src.append(n)
                dst.append(d)
    info = {'seed': SEED, 'degree': DEGREE, 'query_types': QUERY_TYPES,
            'schema': {'modes': schema.modes, 'relations': {m: [list(v) for v in schema.relations[m]] for m in schema.modes},
                       'ids': {m: schema.ids[m].tolist() for m in schema.modes}, 'num_entities': schema.num_entities}}
    neg_off, neg_ids = _csr(neg)
    hard_off, hard_ids = _csr(hard)
    meta_off, meta_ids = _csr(meta)
    np.savez_compressed(OUT, meta=np.frombuffer(json.dumps(info).encode(), dtype=np.uint8),
                        adj_rel=np.array(rel, dtype=np.int64), adj_src=np.array(src, dtype=np.int64),
                        adj_dst=np.array(dst, dtype=np.int64), types=np.array(types, dtype=np.int64),
                        edges=np.stack(edges), none=np.array(none, dtype=np.int64), neg_off=neg_off, neg_ids=neg_ids,
                        hard_off=hard_off, hard_ids=hard_ids, meta_off=meta_off, meta_ids=meta_ids)
    print('%s: %d cases, %d with (None, None), %d bytes' % (OUT, len(cases), sum(none), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
