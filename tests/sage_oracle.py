"""TEST INFRASTRUCTURE ONLY -- csrc/sage.hip restated on the host: the neighbour sampler with Python ints (the stream and the
keyed bijection are tests/kg_sample_oracle.py's, imported, not copied), and the encoder's forward and backward in numpy
float64 from the definition in include/mpqe_amd.h (mpqe_sage_fwd / mpqe_sage_bwd). Nothing here comes from the library or
from mpqe_amd/ops.py.

A world's relations are tests/test_kg_kernels.py's: relations[i] = (source mode, destination mode, {row: [rows]})."""
import math

import numpy as np

from tests.kg_sample_oracle import mix64, permute, slot_base  # noqa: F401  (mix64: for callers that restate a slot)


def keep_count(length, keep_prob, max_keep):
    """aggregators.py:51-53, the reference's own expression"""
    return min(int(math.ceil(length * keep_prob)), max_keep)


def sample_neighbours(relations, use_rels, rows, keep_prob, max_keep, seed):
    """what mpqe_kg_sample_neighbours writes -> (neigh [R, B, max_keep] int64, counts [R, B] int32)"""
    R, B = len(use_rels), len(rows)
    neigh = np.full((R, B, max_keep), -1, dtype=np.int64)
    counts = np.zeros((R, B), dtype=np.int32)
    for i, ri in enumerate(use_rels):
        lists = relations[ri][2]
        for b, x in enumerate(rows):
            lst = list(lists.get(int(x), ())) if x >= 0 else []
            if not lst:
                continue
            k = keep_count(len(lst), keep_prob, max_keep)
            if k == len(lst):
                picks = lst
            else:
                key = slot_base(seed, (int(ri) << 32) | b)
                picks = [lst[permute(key, len(lst), j)] for j in range(k)]
            neigh[i, b, :k] = picks
            counts[i, b] = k
    return neigh, counts


def _row(table, row):
    """a row outside the table reads as zeros"""
    return table[row] if 0 <= row < table.shape[0] else np.zeros(table.shape[1])


def features(tables, block_table, block_pad, neigh, counts, self_rows):
    """[B, (R + 1) din] float64: the mean rows of every relation block in slot order, then the self rows"""
    R, B = counts.shape[0], len(self_rows)
    din = tables[0].shape[1]
    feat = np.zeros((B, (R + 1) * din))
    for r in range(R):
        t = np.asarray(tables[block_table[r]], dtype=np.float64)
        for b in range(B):
            c = int(counts[r, b])
            if c == 0:
                v = t[block_pad[r]]
            else:
                v = sum(_row(t, int(neigh[r, b, s])) for s in range(c)) / c
            feat[b, r * din:(r + 1) * din] = v
    t = np.asarray(tables[block_table[R]], dtype=np.float64)
    for b in range(B):
        row = int(self_rows[b])
        feat[b, R * din:] = _row(t, block_pad[R] if row < 0 else row)
    return feat


def forward(tables, block_table, block_pad, neigh, counts, self_rows, W, gamma=None, beta=None, eps=1e-6):
    """-> dict: feat, z, pre (what the ReLU sees), out, and the normalisation's mean / std"""
    feat = features(tables, block_table, block_pad, neigh, counts, self_rows)
    z = feat @ np.asarray(W, dtype=np.float64).T
    st = {'feat': feat, 'z': z}
    if gamma is None:
        pre = z
    else:
        mean = z.mean(axis=1, keepdims=True)
        std = z.std(axis=1, ddof=1, keepdims=True)
        st.update(mean=mean, std=std)
        pre = np.asarray(gamma, dtype=np.float64) * (z - mean) / (std + eps) + np.asarray(beta, dtype=np.float64)
    st['pre'] = pre
    st['out'] = np.maximum(pre, 0.0)
    return st


def backward(tables, block_table, block_pad, neigh, counts, self_rows, W, grad_out, gamma=None, beta=None, eps=1e-6, st=None):
    """-> (grad_tables [one per table, zeros where untouched], grad_W, grad_gamma, grad_beta) in float64"""
    if st is None:
        st = forward(tables, block_table, block_pad, neigh, counts, self_rows, W, gamma, beta, eps)
    W = np.asarray(W, dtype=np.float64)
    g = np.asarray(grad_out, dtype=np.float64) * (st['pre'] > 0)
    grad_gamma = grad_beta = None
    if gamma is None:
        gz = g
    else:
        gamma = np.asarray(gamma, dtype=np.float64)
        z, mean, std = st['z'], st['mean'], st['std']
        D = z.shape[1]
        s = std + eps
        xc = z - mean
        grad_gamma, grad_beta = (g * xc / s).sum(axis=0), g.sum(axis=0)
        d = g * gamma
        gz = (d - d.mean(axis=1, keepdims=True)) / s - xc * (d * xc).sum(axis=1, keepdims=True) / ((D - 1) * std * s * s)
    grad_W = gz.T @ st['feat']
    gfeat = gz @ W
    R, B = counts.shape[0], len(self_rows)
    din = tables[0].shape[1]
    grads = [np.zeros(np.asarray(t).shape) for t in tables]

    def add(t, row, v):
        if 0 <= row < grads[t].shape[0]:
            grads[t][row] += v
    for r in range(R):
        for b in range(B):
            gr, c = gfeat[b, r * din:(r + 1) * din], int(counts[r, b])
            if c == 0:
                add(block_table[r], block_pad[r], gr)
            for s in range(c):
                add(block_table[r], int(neigh[r, b, s]), gr / c)
    for b in range(B):
        row = int(self_rows[b])
        add(block_table[R], block_pad[R] if row < 0 else row, gfeat[b, R * din:])
    return grads, grad_W, grad_gamma, grad_beta
