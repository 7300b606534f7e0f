"""A float64 numpy restatement of the GQE baseline (reference model.py:57-134, decoders.py:123-150, 270-319,
encoders.py:40-43), forward and backward, the counterpart of tests/dropin_oracle.py for `QueryEncoderDecoder`. The GPU
tests compare against it at shapes the fixtures (tests/golden/gqe_*.npz) do not cover; tests/test_gqe_host.py pins it to
those fixtures.

    o = Oracle(params, node_map)          params keyed like the model's state_dict:
                                            enc.feat-<mode>.weight, path_dec.<a>_<r>_<b>, inter_dec.<mode>_premat / _postmat
    s = o.forward(formula, anchors, targets, negs, neg_lengths, inter)       inter: 'mean' | 'min' | 'mean-simple' | 'min-simple'
    o.backward(grad_scores)               gradients of the LAST forward, added to o.grads (same keys)
    loss = o.margin_loss(formula, anchors, targets, negs, inter, margin)     forward twice + hinge + backward

Embeddings are rows here ([n, D]); the reference's are columns."""
import numpy as np

EPS = 1e-8                        # nn.CosineSimilarity's default, the library's mpqe_cosine_fwd
FWD = dict(rtol=1e-5, atol=1e-6)      # tests/test_configs_gpu.py: scores / loss against the oracle
BWD = dict(rtol=1e-4, atol=2e-6)      # ... every parameter gradient


def reverse(rel):
    return (rel[2], rel[1], rel[0])


def rel_key(rel):
    return 'path_dec.' + '_'.join(rel)


class Oracle(object):
    def __init__(self, params, node_map, dtype=np.float64):
        # (dtype float32: the same op sequence at the kernels' precision -- how far fp32 alone moves a result, see
        # tests/gqe_common.py well_conditioned)
        self.dtype = dtype
        self.p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
        self.node_map = np.asarray(node_map, dtype=np.int64)
        self.grads = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.tape = []
        self.kept = {}

    def zero_grad(self):
        for g in self.grads.values():
            g[...] = 0.0

    # ---- ops: each returns its value and records how a gradient of it flows on
    def embed(self, ids, mode):
        key = 'enc.feat-%s.weight' % mode
        rows = self.node_map[np.asarray(ids, dtype=np.int64)]
        raw = self.p[key][rows]
        nrm = np.linalg.norm(raw, axis=1, keepdims=True)
        y = raw / nrm

        def back(g):
            np.add.at(self.grads[key], rows, (g - y * (y * g).sum(1, keepdims=True)) / nrm)
            return ()
        return self._rec(y, (), back)

    def mm(self, x, key, transposed):
        W = self.p[key]
        y = x.v @ (W.T if transposed else W)

        def back(g):
            if transposed:
                self.grads[key] += g.T @ x.v
                return (g @ W,)
            self.grads[key] += x.v.T @ g
            return (g @ W.T,)
        return self._rec(y, (x,), back)

    def relu(self, x):
        return self._rec(np.maximum(x.v, 0.0), (x,), lambda g: (g * (x.v > 0),))

    def agg(self, xs, kind):
        st = np.stack([x.v for x in xs])
        if kind == 'mean':
            return self._rec(st.mean(0), xs, lambda g: tuple(g / len(xs) for _ in xs))
        win = st.argmin(0)                    # (ties: the lowest branch)
        self.kept['min_gap'] = np.sort(st, axis=0)[1] - np.sort(st, axis=0)[0]
        return self._rec(st.min(0), xs, lambda g: tuple(g * (win == k) for k in range(len(xs))))

    def take(self, x, idx):
        def back(g):
            out = np.zeros_like(x.v)
            np.add.at(out, idx, g)
            return (out,)
        return self._rec(x.v[idx], (x,), back)

    def cos(self, a, b):
        dot = (a.v * b.v).sum(1)
        ra, rb = np.linalg.norm(a.v, axis=1), np.linalg.norm(b.v, axis=1)
        na, nb = np.maximum(ra, EPS), np.maximum(rb, EPS)
        s = dot / (na * nb)

        def back(g):
            inv = (1.0 / (na * nb))[:, None]
            ka = np.where(ra > EPS, s / (na * na), 0.0)[:, None]
            kb = np.where(rb > EPS, s / (nb * nb), 0.0)[:, None]
            return (g[:, None] * (b.v * inv - ka * a.v), g[:, None] * (a.v * inv - kb * b.v))
        return self._rec(s, (a, b), back)

    def _rec(self, v, parents, back):
        node = _Node(v)
        self.tape.append((node, parents, back))
        return node

    # ---- the model
    def project(self, x, rel):
        return self.mm(x, rel_key(rel), True)                     # decoders.py:150, rows

    def intersect(self, xs, mode, inter):
        kind = inter.split('-')[0]
        if inter.endswith('-simple'):
            return self.agg(xs, kind)
        pre, post = 'inter_dec.%s_premat' % mode, 'inter_dec.%s_postmat' % mode
        preact = [self.mm(x, pre, True) for x in xs]
        self.kept['preact'] = [h.v for h in preact]
        hidden = [self.relu(h) for h in preact]
        return self.mm(self.agg(hidden, kind), post, True)

    def forward(self, formula, anchors, targets, negs=None, neg_lengths=None, inter='mean'):
        """scores [B (+ sum(neg_lengths))]: model.py:70-116. anchors [B, A]."""
        self.tape, self.kept = [], {}
        anchors = np.asarray(anchors, dtype=np.int64).reshape(len(targets), -1)
        tnodes = np.asarray(targets, dtype=np.int64)
        qrow = np.arange(len(targets))
        if negs is not None:
            tnodes = np.concatenate([tnodes, np.asarray(negs, dtype=np.int64)])
            qrow = np.concatenate([qrow, np.repeat(np.arange(len(targets)), np.asarray(neg_lengths, dtype=np.int64))])
        qt, rels = formula.query_type, formula.rels
        t = self.embed(tnodes, formula.target_mode)
        if qt in ('1-chain', '2-chain', '3-chain'):
            act = t
            for rel in rels:
                act = self.mm(act, rel_key(tuple(rel)), False)          # decoders.py:143-145
            a = self.take(self.embed(anchors[:, 0], formula.anchor_modes[0]), qrow)
            out = self.cos(act, a)
        else:
            if qt == '3-chain_inter':
                e1 = self.project(self.embed(anchors[:, 0], formula.anchor_modes[0]), reverse(rels[1][0]))
                e2 = self.project(self.embed(anchors[:, 1], formula.anchor_modes[1]), reverse(rels[1][1]))
                q = self.intersect([e1, e2], rels[0][-1], inter)
                q = self.project(q, reverse(rels[0]))
            else:
                xs = [self.project(self.embed(anchors[:, 0], formula.anchor_modes[0]), reverse(rels[0]))]
                e2 = self.embed(anchors[:, 1], formula.anchor_modes[1])
                if len(rels[1]) == 2:
                    for r in rels[1][::-1]:
                        e2 = self.project(e2, reverse(r))
                else:
                    e2 = self.project(e2, reverse(rels[1]))
                xs.append(e2)
                if qt == '3-inter':
                    xs.append(self.project(self.embed(anchors[:, 2], formula.anchor_modes[2]), reverse(rels[2])))
                q = self.intersect(xs, formula.target_mode, inter)
            out = self.cos(t, self.take(q, qrow))
        self.out = out
        return out.v

    def backward(self, grad_scores):
        for node, _, _ in self.tape:
            node.g = None
        self.out.g = np.asarray(grad_scores, dtype=self.dtype)
        for node, parents, back in reversed(self.tape):
            if node.g is None:
                continue
            for p, g in zip(parents, back(node.g)):
                p.g = g if p.g is None else p.g + g

    def margin_loss(self, formula, anchors, targets, negs, inter='mean', margin=1.0):
        """model.py:129-134 (the negatives are the caller's); gradients are added to self.grads."""
        n = len(targets)
        pos = self.forward(formula, anchors, targets, inter=inter)
        tape_pos, out_pos = self.tape, self.out
        neg = self.forward(formula, anchors, negs, inter=inter)
        h = margin - (pos - neg)
        loss = np.maximum(h, 0.0).mean()
        g = (h > 0) / float(n)
        self.backward(g)                   # d loss / d neg
        self.tape, self.out = tape_pos, out_pos
        self.backward(-g)
        self.hinge = h
        return loss


class _Node(object):
    __slots__ = ('v', 'g')

    def __init__(self, v):
        self.v, self.g = v, None
