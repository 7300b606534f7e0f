"""TEST INFRASTRUCTURE ONLY -- the exact answers of a conjunctive query as Python sets: synthetic._answers restated, plus
the union flavour the hard negatives come from (reference Graph.get_negative_samples, graph.py:263-314: negatives =
full_sets[target mode] - answers; hard negatives = union of the branch sets - their intersection, for 3-chain_inter both
pushed through the last relation first). tests/test_kg_host.py pins it to sets the reference itself produced
(tests/golden/kg_sets_small.npz); everywhere else it is the oracle of csrc/kg.hip.

A hop is anything with .get(row, default) -> iterable of rows: a dict of sets (adj_lists[rel]) or a dict of lists."""
from mpqe_amd.graph import reverse_relation


def hop_set(hop, nodes):
    """the union of the lists of `nodes`; a node without a list contributes nothing (graph.py:467)"""
    out = set()
    for x in nodes:
        out |= set(hop.get(x, ()))
    return out


def programme_sets(branches, tail, anchors):
    """branches: per branch the hops from its anchor; tail: the hops after the merge; anchors: one per branch.
    -> (merge taken as AND, merge taken as OR), both after the tail."""
    sets = []
    for hops, a in zip(branches, anchors):
        s = {a}
        for h in hops:
            s = hop_set(h, s)
        sets.append(s)
    both, some = set.intersection(*sets), set.union(*sets)
    for h in tail:
        both, some = hop_set(h, both), hop_set(h, some)
    return both, some


def formula_hops(formula):
    """([(anchor slot, [relation walked per hop])], [relations after the merge]): every query edge (x, rel, y) is walked
    from y to x, along reverse_relation(rel)"""
    qt, rels = formula.query_type, formula.rels
    rev = reverse_relation
    if qt.endswith('-chain'):
        return [(0, [rev(r) for r in reversed(rels)])], []
    if qt.endswith('-inter'):
        return [(i, [rev(r)]) for i, r in enumerate(rels)], []
    if qt == '3-inter_chain':
        return [(0, [rev(rels[0])]), (1, [rev(rels[1][1]), rev(rels[1][0])])], []
    assert qt == '3-chain_inter'
    return [(0, [rev(rels[1][0])]), (1, [rev(rels[1][1])])], [rev(rels[0])]


def query_sets(adj, formula, anchors):
    """(answers, hard negatives) of one query on adj_lists `adj`, as sets of entity ids"""
    branches, tail = formula_hops(formula)
    both, some = programme_sets([[adj[tuple(r)] for r in hops] for _, hops in branches], [adj[tuple(r)] for r in tail],
                                [anchors[slot] for slot, _ in branches])
    return both, some - both


def negatives(adj, full_set, formula, anchors):
    """(full_set - answers, hard negatives)"""
    ans, hard = query_sets(adj, formula, anchors)
    return set(full_set) - ans, hard
