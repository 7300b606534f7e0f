"""tests/gqe_common.py extended to the two vector path decoders: the fixtures tests/golden/vecdec_*.npz as models /
oracles, random problems whose path parameters are [D] vectors, and the same driver of mpqe_gqe_fwd / mpqe_gqe_bwd
(gqe_common.Call) with the programme's operator and score ints set."""
import os

import numpy as np

from tests import gqe_common as gc
from tests.conftest import CaseGraph, golden_paths
from tests.gqe_oracle import BWD, FWD
from tests.gqe_vec_oracle import CHAINS, DECODERS, VecOracle

OP = {'transe': 1, 'bilinear-diag': 2}           # programme int [7]


def case_paths():
    return golden_paths('vecdec_')


def case_ids():
    return [os.path.basename(p)[:-4] for p in case_paths()]


def case_oracle(case):
    return VecOracle({k: v.numpy() for k, v in case.params().items()}, case.arrays['node_map'], case.cfg['decoder'])


def build_model(case, device=None, fused=True):
    """gqe_common.build_model with the fixture's path decoder (get_metapath_decoder's keyword)."""
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.model import QueryEncoderDecoder
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    feature_modules, node_maps = make_feature_modules(case.ids, case.D, case.num_entities)
    graph = CaseGraph(case)
    enc = DirectEncoder(None, feature_modules, node_maps)
    dims = {m: case.D for m in case.modes}
    model = QueryEncoderDecoder(graph, enc, get_metapath_decoder(graph, dims, case.cfg['decoder'], vector_decoders=True),
                                get_intersection_decoder(graph, dims, case.cfg['inter']))
    model.load_state_dict(case.params(), strict=True)
    model.fused = fused
    return model if device is None else model.to(device)


class VecProblem(gc.Problem):
    """gqe_common.Problem with one [D] vector per relation, drawn as the decoders initialise theirs
    (uniform(-6 / sqrt(D), 6 / sqrt(D)), decoders.py:196), after everything the base class draws."""

    def __init__(self, decoder, query_type, D, B, inter, seed, repeat=False, rows=23):
        assert decoder in DECODERS
        super(VecProblem, self).__init__(query_type, D, B, inter, seed, repeat, rows)
        self.decoder = decoder
        rng = np.random.RandomState(seed + 7919)
        lim = 6.0 / np.sqrt(D)
        for k in sorted(self.params):
            if k.startswith('path_dec.'):
                self.params[k] = rng.uniform(-lim, lim, D).astype(np.float32)

    def _oracle(self, dtype, jitter=None):
        o = VecOracle(self.params, self.node_map, self.decoder, dtype=dtype, jitter=jitter)
        s = o.forward(self.formula, self.anchors, self.targets, self.negs, self.neg_lengths, self.inter)
        o.backward(self.grad_scores)
        return o, s

    def oracle(self):
        return self._oracle(np.float64)

    def well_conditioned(self, o, scores):
        """gqe_common.Problem.well_conditioned with the extended oracle -- its own op sequence in float32 (numpy) must
        stay within half of FWD / BWD of the float64 one -- and a second probe: the float64 oracle with every op's result
        shaken by up to one fp32 ulp (VecOracle jitter, two draws) must stay within half of them too.
        Why the second: the vectors are drawn as the decoders initialise them, up to 6 / sqrt(D) per entry, so rows and
        gradients are several times the bilinear problems', against the same absolute tolerance. A matrix-gradient entry
        that cancels to 1e-3 over the batch while its terms are of order 1 then moves by several 1e-6 under ONE ulp per
        op; numpy's float32 run happens to round kindly there (wide accumulators, fused multiply-adds) and says nothing
        about another order of the same operations, which is what a kernel is. A draw that one ulp per op takes half way
        to the tolerance cannot test a kernel at it. Read from the oracle alone, never from the code under test."""
        def within(a, b, tol):
            return bool((np.abs(a - b) <= 0.5 * (tol['atol'] + tol['rtol'] * np.abs(b))).all())
        o32, s32 = self._oracle(np.float32)
        if not (within(s32, scores, FWD) and all(within(o32.grads[k], o.grads[k], BWD) for k in o.grads)):
            return False
        for draw in range(2):
            oj, sj = self._oracle(np.float64, jitter=np.random.RandomState(draw))
            if not (within(sj, scores, FWD) and all(within(oj.grads[k], o.grads[k], BWD) for k in o.grads)):
                return False
        return True


def settled_problem(decoder, query_type, D, B, inter, seed, repeat=False, tweak=None):
    """gqe_common.settled_problem's rules on a VecProblem: the first seed from `seed` on without a near-tie and well
    conditioned, both judged from the oracle alone."""
    for s in range(seed, seed + 50):
        prob = VecProblem(decoder, query_type, D, B, inter, s, repeat)
        if tweak is not None:
            tweak(prob)
        o, scores = prob.oracle()
        if prob.near_ties(o) == 0 and prob.well_conditioned(o, scores):
            return prob, o, scores
    raise AssertionError('no seed without near-ties')


def pack(prob):
    """gqe_common.pack with the operator ([7]) and, on a chain under the diagonal decoder, the dot score ([27]) set."""
    packed = list(gc.pack(prob))
    prog = np.array(packed[0], dtype=np.int32)
    prog[7] = OP[prob.decoder]
    prog[27] = int(prob.decoder == 'bilinear-diag' and prob.formula.query_type in CHAINS)
    packed[0] = prog
    return tuple(packed)


def call(be, prob, packed=None):
    return gc.Call(be, prob, packed if packed is not None else pack(prob))
