"""TEST INFRASTRUCTURE ONLY, run where a checkout of the reference exists -- generates tests/golden/kg_walks_small.npz by
IMPORTING the reference's Graph and calling its own Graph.sample_query_subgraph_bytype TRIES times per query type under a
fixed random.seed, on a tiny graph that is closed under inverse (so the reference's sample_edge never meets an empty
list). Only the graph and the recorded counts are written.

    MPQE_REFERENCE=<checkout of the reference> python tools/gen_kg_walk_golden.py

The fixture: meta (JSON: modes, ids per mode, the typed relations in index order, tries, seed), the graph as arrays
(adj_rel = index into the typed relations, adj_src, adj_dst; both directions of every edge), and per query type t = 1 .. 6
(2-chain .. 3-chain_inter; the reference's walk has no 1-chain) out_t [U, 9] = the distinct outcomes, each the query
tuple's edges (node, relation index, node) with nested tuples flattened and -1 padded, None as a row of -1, and cnt_t [U]
how often each came up. The adjacency handed to the reference holds a node as a key only where it has an edge, as the
start of its walk draws among the keys.
"""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get('MPQE_REFERENCE', '')
OUT = os.path.join(ROOT, 'tests', 'golden', 'kg_walks_small.npz')

QUERY_TYPES = ['1-chain', '2-chain', '3-chain', '2-inter', '3-inter', '3-inter_chain', '3-chain_inter']
SEED, TRIES = 23, 20000
MODES = {'a': list(range(0, 6)), 'b': list(range(6, 13)), 'c': list(range(13, 18))}
FORWARD = [(('a', 'r0', 'b'), 7), (('a', 'r1', 'b'), 4), (('b', 'r2', 'c'), 7), (('c', 'r3', 'a'), 5)]     # (relation, edges)


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


def main():
    if not os.path.isdir(os.path.join(REF, 'mpqe')):
        raise SystemExit('set MPQE_REFERENCE to a checkout of the reference (found none at %r)' % REF)
    sys.path.insert(0, REF)
    import mpqe.graph as rgraph
    rng = np.random.RandomState(SEED)
    typed, adj = [], {}
    for rel, _ in FORWARD:
        typed += [rel, rgraph._reverse_relation(rel)]
    typed = [tuple(r) for r in typed]
    for rel in typed:
        adj[rel] = {}
    for rel, count in FORWARD:
        inv = tuple(rgraph._reverse_relation(rel))
        src, dst = MODES[rel[0]], MODES[rel[2]]
        pairs = rng.choice(len(src) * len(dst), size=count, replace=False)
        for p in pairs:
            s, d = src[int(p) // len(dst)], dst[int(p) % len(dst)]
            adj[rel].setdefault(s, set()).add(d)
            adj[inv].setdefault(d, set()).add(s)
    relations = {m: [] for m in MODES}
    for (m1, name, m2) in typed:
        relations[m1].append((m2, name))
    graph = rgraph.Graph(None, {m: 1 for m in MODES}, relations, adj)
    rel_index = {r: i for i, r in enumerate(typed)}
    arrays = {}
    for t in range(1, len(QUERY_TYPES)):
        random.seed(SEED * 100 + t)
        counts = {}
        for _ in range(TRIES):
            q = graph.sample_query_subgraph_bytype(QUERY_TYPES[t])
            key = (-1,) * 9
            if q is not None:
                assert q[0] == QUERY_TYPES[t]
                flat = [v for (x, rel, y) in _flat_edges(q) for v in (x, rel_index[tuple(rel)], y)]
                key = tuple(flat + [-1] * (9 - len(flat)))
            counts[key] = counts.get(key, 0) + 1
        keys = sorted(counts)
        arrays['out_%d' % t] = np.array(keys, dtype=np.int64).reshape(-1, 9)
        arrays['cnt_%d' % t] = np.array([counts[k] for k in keys], dtype=np.int64)
    rel, src, dst = [], [], []
    for r in typed:
        for n in sorted(adj[r]):
            for d in sorted(adj[r][n]):
                rel.append(rel_index[r])
                src.append(n)
                dst.append(d)
    info = {'seed': SEED, 'tries': TRIES, 'query_types': QUERY_TYPES, 'modes': list(MODES), 'ids': MODES,
            'typed_relations': [list(r) for r in typed]}
    np.savez_compressed(OUT, meta=np.frombuffer(json.dumps(info).encode(), dtype=np.uint8),
                        adj_rel=np.array(rel, dtype=np.int64), adj_src=np.array(src, dtype=np.int64),
                        adj_dst=np.array(dst, dtype=np.int64), **arrays)
    print('%s: %d directed edges, %s distinct outcomes per type, %d bytes'
          % (OUT, len(rel), [int(arrays['cnt_%d' % t].shape[0]) for t in range(1, 7)], os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
