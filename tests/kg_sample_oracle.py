"""TEST INFRASTRUCTURE ONLY -- csrc/kg_sample.hip restated with Python ints: the counter-based stream (include/mpqe_amd.h,
"The random stream"), the walk of mpqe_kg_sample_queries, the keyed bijection of mpqe_kg_sample_rows; and, independent of
any stream, the EXACT single-try distribution of the reference's walk (Graph.sample_query_subgraph_bytype,
graph.py:321-389) by enumerating its tree, with the chi-square statistic the tests put observed counts through.
tests/test_kg_sample_kernels.py pins the enumeration to counts the reference itself produced
(tests/golden/kg_walks_small.npz).

A world is (mode_rows, relations): relations[i] = (source mode, destination mode, {row: [rows]}), lists as given (repeats
allowed), everything in rows."""
import math
from fractions import Fraction

import numpy as np

M64 = (1 << 64) - 1
MAX_REDRAWS = 64                # KGS_MAX_REDRAWS
FEISTEL_ROUNDS = 8              # KGS_FEISTEL_ROUNDS
QUERY_TYPES = ['1-chain', '2-chain', '3-chain', '2-inter', '3-inter', '3-inter_chain', '3-chain_inter']
# per type: (entries needed at the start, [(edge whose neighbour is walked on from, entries needed there)])
SHAPES = {0: (1, []), 1: (1, [(0, 1)]), 2: (1, [(0, 1), (1, 1)]), 3: (2, []), 4: (3, []), 5: (2, [(1, 1)]), 6: (1, [(0, 2)])}


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def slot_base(seed, slot):
    return mix64((seed & M64) ^ mix64(slot))


# ---------------------------------------------------------------------------------------------- the walk
def flat_list(relations, mode, x):
    """[(relation index, neighbour)]: x's lists in every relation out of `mode`, in relation-index order"""
    return [(i, y) for i, (src, _, lists) in enumerate(relations) if src == mode for y in lists.get(x, ())]


class _Draws(object):
    def __init__(self, key):
        self.key, self.d = key, 0

    def next(self, length):
        r = mix64(self.key ^ self.d) % length
        self.d += 1
        return r


def _edges_out(relations, draws, at, mode, fan, edges):
    flat = flat_list(relations, mode, at)
    if len(flat) < fan:
        return False
    mine = []
    for _ in range(fan):
        redraws = 0
        while True:
            pick = flat[draws.next(len(flat))]
            if pick not in mine:
                break
            redraws += 1
            if redraws >= MAX_REDRAWS:
                return False
        mine.append(pick)
        edges.append((at, pick[0], pick[1]))
    return True


def walk_try(relations, qt, draws):
    """one try -> [(source row, relation, destination row)] or None"""
    active = [i for i, (_, _, lists) in enumerate(relations) if any(len(l) for l in lists.values())]
    if not active:
        return None
    r0 = active[draws.next(len(active))]
    starts = sorted(x for x, l in relations[r0][2].items() if len(l))
    x = starts[draws.next(len(starts))]
    first, then = SHAPES[qt]
    edges = []
    if not _edges_out(relations, draws, x, relations[r0][0], first, edges):
        return None
    for frm, fan in then:
        _, rel, y = edges[frm]
        if not _edges_out(relations, draws, y, relations[rel][1], fan, edges):
            return None
    return edges


def walk(relations, qt, Q, max_tries, seed):
    """out [Q, 10] of mpqe_kg_sample_queries"""
    out = np.full((Q, 10), -1, dtype=np.int64)
    for q in range(Q):
        base = slot_base(seed, q)
        out[q, 0] = 0
        for t in range(max_tries):
            edges = walk_try(relations, qt, _Draws(mix64(base ^ t)))
            if edges is not None:
                out[q, 0] = 1
                out[q, 1:1 + 3 * len(edges)] = [v for e in edges for v in e]
                break
    return out


# ---------------------------------------------------------------------------------------------- exact distribution
def _fan_outcomes(flat, fan):
    """{tuple of `fan` picks: probability}: each pick uniform over the entries, redrawn until its (relation, neighbour)
    differs from the earlier picks' (an unbounded redraw: the kernel's bound of 64 changes a probability by at most
    (2/3)^64 on the worlds here). The missing mass, if no entry differs, is a rejection."""
    out = {(): Fraction(1)}
    for _ in range(fan):
        nxt = {}
        for picks, p in out.items():
            ok = [e for e in flat if e not in picks]
            for e in ok:
                nxt[picks + (e,)] = nxt.get(picks + (e,), 0) + p / len(ok)
        out = nxt
    return out


def single_try_distribution(relations, qt):
    """{outcome: Fraction}: outcome = tuple of edges (source, relation, destination) flattened, or None"""
    active = [i for i, (_, _, lists) in enumerate(relations) if any(len(l) for l in lists.values())]
    dist = {}
    first, then = SHAPES[qt]

    def extend(edges, p, steps):
        if not steps:
            key = tuple(v for e in edges for v in e)
            dist[key] = dist.get(key, 0) + p
            return
        (frm, fan), rest = steps[0], steps[1:]
        _, rel, y = edges[frm]
        flat = flat_list(relations, relations[rel][1], y)
        if len(flat) < fan:
            return
        for picks, pp in _fan_outcomes(flat, fan).items():
            extend(edges + [(y, r, z) for r, z in picks], p * pp, rest)

    for r0 in active:
        starts = sorted(x for x, l in relations[r0][2].items() if len(l))
        for x in starts:
            p = Fraction(1, len(active) * len(starts))
            flat = flat_list(relations, relations[r0][0], x)
            if len(flat) < first:
                continue
            for picks, pp in _fan_outcomes(flat, first).items():
                extend([(x, r, z) for r, z in picks], p * pp, then)
    dist[None] = 1 - sum(dist.values())
    if dist[None] == 0:
        del dist[None]
    return dist


def _gammaincc(a, x):
    """regularised upper incomplete gamma Q(a, x) (series below a + 1, continued fraction above)"""
    if x <= 0:
        return 1.0
    lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1:
        term = total = 1.0 / a
        n = a
        for _ in range(10000):
            n += 1
            term *= x / n
            total += term
            if abs(term) < abs(total) * 1e-16:
                break
        return 1.0 - total * lead
    tiny = 1e-300
    b = x + 1 - a
    c, d = 1 / tiny, 1 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1 / d
        delta = d * c
        h *= delta
        if abs(delta - 1) < 1e-16:
            break
    return lead * h


def chi_square(observed, dist, total):
    """Pearson's statistic of observed {outcome: count} against dist {outcome: probability} over `total` draws; outcomes of
    expected count < 5 are pooled into one cell. An observed outcome the distribution does not know is an outright failure
    (p = 0). -> (statistic, degrees of freedom, p)"""
    if any(k not in dist for k in observed) or sum(observed.values()) != total:
        return float('inf'), 0, 0.0
    cells, pool_e, pool_o = [], 0.0, 0
    for k, p in dist.items():
        e = float(p) * total
        o = observed.get(k, 0)
        if e < 5:
            pool_e += e
            pool_o += o
        else:
            cells.append([e, o])
    if pool_e >= 5 or not cells:
        cells.append([pool_e, pool_o])
    elif pool_e > 0:                 # a pool too small for a cell of its own joins the smallest cell
        cells.sort()
        cells[0][0] += pool_e
        cells[0][1] += pool_o
    stat = sum((o - e) ** 2 / e for e, o in cells if e > 0)
    dof = max(len(cells) - 1, 1)
    return stat, dof, _gammaincc(dof / 2.0, stat / 2.0)


def counts_of(records):
    """{outcome: count} of a [Q, 10] array (status 0 -> None)"""
    out = {}
    for rec in np.asarray(records):
        key = None if rec[0] == 0 else tuple(int(v) for v in rec[1:] if v >= 0)
        out[key] = out.get(key, 0) + 1
    return out


# ---------------------------------------------------------------------------------------------- at most k rows
def permute(key, c, j):
    h = 1
    while (1 << (2 * h)) < c:
        h += 1
    mask = (1 << h) - 1
    x = j
    while True:
        L, R = x >> h, x & mask
        for r in range(FEISTEL_ROUNDS):
            L, R = R, L ^ (mix64(key ^ (((r + 1) << 32) | R)) & mask)
        x = (L << h) | R
        if x < c:
            return x


def sample_rows(members, k, seed, q):
    """what mpqe_kg_sample_rows writes for query q whose selected set is `members` (ascending rows)"""
    c = len(members)
    if c <= k:
        return list(members)
    key = slot_base(seed, q)
    return [members[permute(key, c, j)] for j in range(k)]
