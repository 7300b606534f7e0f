"""The R-GCN model over a window of queries of DIFFERENT formulas of one query type in plain torch on the CPU, written from
the formulas of include/mpqe_amd.h: lookup (node_map, a bad id's row is zeros), x / |x|, the mode-embedding rows, per pass
out[:, n] = sum over the edges into n of h[:, src] @ basis[rel] + h[:, n] @ root + bias with a ReLU after every pass but
the last, the readout (target slot / sum / max with the lowest node on ties), the cosine with max(norm, eps). Run by run
over formula_runs, the gradients by autograd, accumulating over the runs. `dtype` float64 is the oracle, float32 its twin.

A problem is a tests/test_rgcn_mixed_kernels.Problem; the window's operands may be replaced (formula_of, anchors,
pair_ids), as may the relation count (a relation at or past it makes its formula contribute nothing, as does a formula
index outside the records)."""
import numpy as np
import torch

from mpqe_amd.model import formula_runs
from tests import gqe_common as gc

EPS = 1e-8


def _lookup(table, node_map, ids, dtype):
    """rows [len(ids), D] of a table by id; a bad id's row is None-marked: (rows clamped, ok mask)"""
    ids = np.asarray(ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < node_map.shape[0])
    rows = np.where(ok, node_map[np.clip(ids, 0, node_map.shape[0] - 1)], -1)
    ok &= (rows >= 0) & (rows < table.shape[0])
    return torch.as_tensor(np.where(ok, rows, 0)), torch.as_tensor(ok)


def _normalised(table, node_map, ids, dtype):
    rows, ok = _lookup(table, node_map, ids, dtype)
    v = table[rows]
    # (a bad id never divides: its row is replaced before the norm)
    safe = torch.where(ok[:, None], v, torch.ones_like(v))
    y = safe / safe.pow(2).sum(1, keepdim=True).sqrt()
    return torch.where(ok[:, None], y, torch.zeros_like(y))


class Result(object):
    pass


def run(prob, dtype=np.float64, grad_scores=None, grad_q=None, formula_of=None, anchors=None, pair_ids=None, R=None,
        recs=None):
    """-> Result: scores [n], q [Q, D], grads {name: array} (when a gradient is given), ties (queries with a ReLU
    pre-activation or a max-readout gap within gc.TIE_TOL), biggest (the largest |value| met: the exact problems')"""
    td = torch.float64 if dtype == np.float64 else torch.float32
    formula_of = prob.formula_of if formula_of is None else np.asarray(formula_of)
    anchors = prob.anchors if anchors is None else anchors
    pair_ids = prob.pair_ids if pair_ids is None else pair_ids
    recs = prob.recs if recs is None else recs
    info = (prob.A, prob.V, prob.N, prob.E)
    A, V, N, E = info
    from tests.test_rgcn_mixed_kernels import template
    tinfo = template(prob.qt)
    src, dst = list(tinfo.src)[:E], list(tinfo.dst)[:E]
    leaf = lambda a: torch.tensor(np.asarray(a), dtype=td, requires_grad=True)
    tables = [leaf(t) for t in prob.tables]
    mode_emb = leaf(prob.mode_emb)
    layers = [(leaf(b), leaf(r), None if bi is None else leaf(bi)) for b, r, bi in prob.layers]
    n_rel = prob.layers[0][0].shape[0] if R is None else R
    Q, D = prob.Q, prob.D
    scores = torch.zeros(prob.n, dtype=td)
    q_all = torch.zeros((Q, D), dtype=td)
    ties, biggest = 0, 0.0
    losses = []
    for f, lo, hi in formula_runs(formula_of):
        if not 0 <= f < recs.shape[0]:
            continue
        rec, B = recs[f], hi - lo
        if any(not 0 <= rec[e] < n_rel for e in range(E)):
            continue
        rows = []
        for a in range(A):
            rows.append(_normalised(tables[rec[3 + a]], prob.node_map, anchors[lo:hi, a], td))
        for k in range(V):
            rows.append(mode_emb[int(rec[6 + k])].expand(B, D))
        h = torch.stack(rows, dim=1)                    # [B, N, D]
        bad = np.zeros(B, dtype=bool)
        for p in range(prob.passes):
            basis, root, bias = layers[prob.layer_of_pass[p]]
            out = []
            for n in range(N):
                acc = h[:, n] @ root
                for e in range(E):
                    if dst[e] == n:
                        acc = acc + h[:, src[e]] @ basis[int(rec[e])]
                if bias is not None:
                    acc = acc + bias
                out.append(acc)
            pre = torch.stack(out, dim=1)
            if p < prob.passes - 1:
                bad |= (pre.detach().abs() <= gc.TIE_TOL).reshape(B, -1).any(1).numpy()
                h = torch.relu(pre)
            else:
                h = pre
            biggest = max(biggest, float(h.detach().abs().max()))
        if prob.readout == 'mp':
            q = h[:, A]
        elif prob.readout == 'sum':
            q = h[:, 0]
            for n in range(1, N):
                q = q + h[:, n]
        else:
            q = h[:, 0]
            for n in range(1, N):
                q = torch.where(h[:, n] > q, h[:, n], q)
            top = torch.sort(h.detach(), dim=1, descending=True)[0]
            gap = (top[:, 0] - top[:, 1]).numpy()
            bad |= ((gap > 0) & (gap <= gc.TIE_TOL)).any(1)
        ties += int(bad.sum())
        q_all[lo:hi] = q.detach()
        if grad_q is not None:
            losses.append((q * torch.as_tensor(np.asarray(grad_q[lo:hi]), dtype=td)).sum())
        a0, b0 = int(prob.neg_off[lo]), int(prob.neg_off[hi])
        ids = np.concatenate([pair_ids[lo:hi], pair_ids[Q + a0:Q + b0]])
        qrow = torch.as_tensor(np.concatenate([np.arange(B), np.repeat(np.arange(B), prob.neg_lengths[lo:hi])]))
        t = _normalised(tables[rec[9]], prob.node_map, ids, td)
        qq = q[qrow]
        s = (qq * t).sum(1) / (qq.pow(2).sum(1).sqrt().clamp(min=EPS) * t.pow(2).sum(1).sqrt().clamp(min=EPS))
        scores[lo:hi] = s.detach()[:B]
        scores[Q + a0:Q + b0] = s.detach()[B:]
        if grad_scores is not None:
            g = np.concatenate([grad_scores[lo:hi], grad_scores[Q + a0:Q + b0]])
            losses.append((s * torch.as_tensor(g, dtype=td)).sum())
    out = Result()
    out.scores, out.q, out.ties, out.biggest = scores.numpy(), q_all.numpy(), ties, biggest
    out.grads = {}
    if losses:
        torch.stack(losses).sum().backward()
    if grad_scores is not None or grad_q is not None:
        z = lambda t: np.zeros(tuple(t.shape), dtype=dtype) if t.grad is None else t.grad.numpy()
        for m, t in enumerate(tables):
            out.grads['table%d' % m] = z(t)
        out.grads['mode_emb'] = z(mode_emb)
        for l, (b, r, bi) in enumerate(layers):
            out.grads['basis%d' % l], out.grads['root%d' % l] = z(b), z(r)
            if bi is not None:
                out.grads['bias%d' % l] = z(bi)
    return out
