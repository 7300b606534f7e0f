"""The float64 oracle of tests/gqe_oracle.py extended by the GQE baseline's two vector path decoders (reference
decoders.py:181-236): TransE (a relation translates, `x + v`) and the diagonal bilinear form (a relation scales, `x * v`,
and a chain is scored by the plain dot product, decoders.py:228-233). Every other op -- lookup and normalisation, the
intersection, the cosine of the intersection forms -- is the base class's. tests/test_gqe_vec_host.py pins it to the
fixtures the reference wrote (tests/golden/vecdec_*.npz, tools/gen_gqe_vec_golden.py).

    o = VecOracle(params, node_map, decoder)      decoder: 'transe' | 'bilinear-diag'; params['path_dec.<a>_<r>_<b>'] is [D]
"""
import numpy as np

from tests.gqe_oracle import Oracle

DECODERS = ('transe', 'bilinear-diag')
CHAINS = ('1-chain', '2-chain', '3-chain')


class VecOracle(Oracle):
    def __init__(self, params, node_map, decoder, dtype=np.float64, jitter=None):
        """jitter: a numpy RandomState, or None. With one, every op's result -- forward values and the gradients handed
        back -- is multiplied element by element by 1 + u * 2^-23, u uniform in [-1, 1]: each op rounded once more, by up
        to one fp32 ulp, in a random direction. How far that moves a result is what fp32 arithmetic in SOME order of
        operations does to it (tests/gqe_vec_common.py well_conditioned)."""
        assert decoder in DECODERS
        super(VecOracle, self).__init__(params, node_map, dtype)
        self.decoder = decoder
        self.chain = False
        self.jitter = jitter

    def _shake(self, v):
        if self.jitter is None:
            return v
        return v * (1.0 + self.jitter.uniform(-1.0, 1.0, np.shape(v)) * 2.0 ** -23)

    def _rec(self, v, parents, back):
        if self.jitter is None:
            return super(VecOracle, self)._rec(v, parents, back)
        return super(VecOracle, self)._rec(self._shake(v), parents, lambda g: tuple(self._shake(x) for x in back(g)))

    # a path site: the base class reaches every one of them through mm(x, 'path_dec.<rel>', transposed); a vector has no
    # transpose, and sites are applied one after another in the caller's order
    def mm(self, x, key, transposed):
        if not key.startswith('path_dec.'):
            return super(VecOracle, self).mm(x, key, transposed)
        v = self.p[key]
        assert v.ndim == 1
        if self.decoder == 'transe':
            def back(g):
                self.grads[key] += g.sum(0)
                return (g,)
            return self._rec(x.v + v, (x,), back)

        def back(g):
            self.grads[key] += (x.v * g).sum(0)
            return (g * v,)
        return self._rec(x.v * v, (x,), back)

    def dot(self, a, b):
        s = (a.v * b.v).sum(1)
        return self._rec(s, (a, b), lambda g: (g[:, None] * b.v, g[:, None] * a.v))

    # model.py:78-83 hands a chain to path_dec.forward: the diagonal decoder's is the dot product; the intersection forms
    # are scored by the model's own cosine under every decoder (model.py:104, 115)
    def cos(self, a, b):
        if self.chain and self.decoder == 'bilinear-diag':
            return self.dot(a, b)
        return super(VecOracle, self).cos(a, b)

    def forward(self, formula, anchors, targets, negs=None, neg_lengths=None, inter='mean'):
        self.chain = formula.query_type in CHAINS
        return super(VecOracle, self).forward(formula, anchors, targets, negs, neg_lengths, inter)
