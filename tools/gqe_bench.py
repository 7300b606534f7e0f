"""GQE baseline: the fused path (one mpqe_gqe_fwd / mpqe_gqe_bwd launch per formula batch) against the same arithmetic in
plain torch ops on the GPU (F.normalize, mm, relu, min / mean, cosine_similarity), per query type and for the 11-batch
AIFB post-burn-in mix, at B = 512, D = 128 on the AIFB-shaped synthetic KG.

    python tools/gqe_bench.py [--batch-size 512] [--embed-dim 128] [--iters 20] [--rounds 5] [--inter min] [--decoder bilinear]
                                [--composed]

Two things are timed, each from the python call to the end of its device work (device events around a window of
`iters` calls, every call with ids of its own; the windows of the variants alternate, the median over `rounds` is
reported):
  forward     model.forward(formula, queries, targets)                    / the torch composition, no autograd
  loss+bwd    model.margin_loss(formula, queries).backward()              / the torch composition + hinge + backward
The model's per-call read of its error word (model.validate, a host sync) is off unless --validate: the torch composition
has no counterpart, and a training loop synchronises on the loss anyway. Both sides receive the same python lists of ids and pay for their own host work and id upload. --composed adds the
package's own composed path (fused = False) beside them; the baseline is the torch composition. One JSON line per
result, then the table in markdown.
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(args, device):
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.model import QueryEncoderDecoder
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    schema = synthetic.make_schema(*synthetic.KG_SHAPES[args.kg], seed=args.seed)
    torch.manual_seed(args.seed)
    graph = synthetic.SchemaGraph(schema, args.embed_dim)
    graph.full_lists = {m: [int(v) for v in ids] for m, ids in graph.full_lists.items()}
    fm, node_maps = make_feature_modules(schema.ids, args.embed_dim, schema.num_entities)
    dims = {m: args.embed_dim for m in schema.modes}
    model = QueryEncoderDecoder(graph, DirectEncoder(None, fm, node_maps), get_metapath_decoder(graph, dims, args.decoder, vector_decoders=True),
                                get_intersection_decoder(graph, dims, args.inter))
    return schema, model.to(device)


class TorchGQE(object):
    """The reference's op sequence (model.py:70-134) on the model's own parameters, rows instead of columns."""

    def __init__(self, model):
        self.m = model
        self.maps = model.enc.node_maps

    def embed(self, ids, mode):
        rows = self.maps[torch.as_tensor(ids, dtype=torch.long).to(self.maps.device)]
        return F.normalize(self.m.enc.table(mode)[rows], dim=1)

    def step(self, x, rel, transposed):
        """One path site on rows: a matrix product, or the vector decoders' x + v / x * v."""
        dec = self.m.path_dec
        if hasattr(dec, 'vecs'):
            return x + dec.vecs[rel] if dec.op == 'translate' else x * dec.vecs[rel]
        return x.mm(dec.mats[rel].t() if transposed else dec.mats[rel])

    def forward(self, formula, queries, targets):
        from mpqe_amd.model import gqe_plan
        m = self.m
        form, branches, imode, tail, emode = gqe_plan(formula)
        t = self.embed(targets, formula.target_mode)
        if form == 0:
            act = t
            for rel, _ in branches[0][2]:
                act = self.step(act, rel, False)
            anchors = self.embed([q.anchor_nodes[0] for q in queries], emode)
            if getattr(m.path_dec, 'score', 'cosine') == 'dot':
                return (act * anchors).sum(dim=1)
            return F.cosine_similarity(act, anchors, dim=1)
        xs = []
        for slot, mode, steps in branches:
            e = self.embed([q.anchor_nodes[slot] for q in queries], mode)
            for rel, _ in steps:
                e = self.step(e, rel, True)
            xs.append(e)
        if hasattr(m.inter_dec, 'pre_mats'):
            xs = [F.relu(x.mm(m.inter_dec.pre_mats[imode].t())) for x in xs]
        st = torch.stack(xs)
        c = st.min(dim=0)[0] if m.inter_dec.agg_kind == 'min' else st.mean(dim=0)
        if hasattr(m.inter_dec, 'post_mats'):
            c = c.mm(m.inter_dec.post_mats[imode].t())
        for rel, _ in tail:
            c = self.step(c, rel, True)
        return F.cosine_similarity(t, c, dim=1)

    def margin_loss(self, formula, queries, hard_negatives=False, margin=1):
        neg = self.m.sample_negatives(formula, queries, hard_negatives)
        affs = self.forward(formula, queries, [q.target_node for q in queries])
        neg_affs = self.forward(formula, queries, neg)
        return torch.clamp(margin - (affs - neg_affs), min=0).mean()


def window(fn, sets):
    """ms per call over one window: fn(batch set) for every set, device events around the lot."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for s in sets:
        fn(s)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / len(sets)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--kg', default='aifb')
    ap.add_argument('--batch-size', type=int, default=512)
    ap.add_argument('--embed-dim', type=int, default=128)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--inter', default='min')
    ap.add_argument('--decoder', default='bilinear', choices=['bilinear', 'transe', 'bilinear-diag'])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--composed', action='store_true')
    ap.add_argument('--validate', action='store_true',
                    help='keep the model\'s per-call read of its error word (a 4-byte device-to-host copy, i.e. a host sync the '
                         'torch composition does not have); off by default here')
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('gqe_bench: no GPU -- nothing is measured without one')
    from mpqe_amd import synthetic
    device = torch.device('cuda:0')
    schema, model = build(args, device)
    model.validate = args.validate
    plain = TorchGQE(model)
    rng = np.random.RandomState(args.seed + 1)
    types = ['1-chain', '2-chain', '3-chain', '2-inter', '3-inter', '3-inter_chain', '3-chain_inter']
    formulas = {qt: synthetic.sample_formula(schema, qt, rng) for qt in types}
    n_sets = args.warmup + args.iters

    def batch(qt):          # (formula, queries): fresh ids every call
        return formulas[qt], synthetic.sample_queries(schema, formulas[qt], args.batch_size, rng, n_neg=4, n_hard=2)
    pool = {qt: [batch(qt) for _ in range(n_sets)] for qt in types}
    work = {qt: [[(pool[qt][i], False)] for i in range(n_sets)] for qt in types}
    work['mix'] = [[(pool[qt][i], hard) for qt, hard in synthetic.FULL_MIX] for i in range(n_sets)]

    def fwd(m):
        def run(s):
            with torch.no_grad():
                for (f, qs), _ in s:
                    m.forward(f, qs, [q.target_node for q in qs])
        return run

    def loss_bwd(m):
        def run(s):
            model.zero_grad(set_to_none=True)
            total = None
            for (f, qs), hard in s:
                l = m.margin_loss(f, qs, hard_negatives=hard)
                total = l if total is None else total + l
            total.backward()
        return run

    variants = [('fused', model, True), ('torch', plain, None)] + ([('composed', model, False)] if args.composed else [])
    results = {}
    for name, sets in work.items():
        for what, make in (('forward', fwd), ('loss_bwd', loss_bwd)):
            times = {v: [] for v, _, _ in variants}
            for r in range(args.rounds + 1):
                for v, m, fused in variants:                     # alternate the variants inside every round
                    if fused is not None:
                        model.fused = fused
                    random.seed(args.seed + 17)
                    if r == 0:
                        window(make(m), sets[:args.warmup])      # warm-up: every shape of the timed window
                    else:
                        times[v].append(window(make(m), sets[args.warmup:]))
            model.fused = True
            rec = dict(what=what, batch=name, B=args.batch_size, D=args.embed_dim, inter=args.inter, decoder=args.decoder, iters=args.iters,
                       rounds=args.rounds)
            for v in times:
                rec[v + '_us'] = 1000.0 * float(np.median(times[v]))
                rec[v + '_us_min_max'] = [1000.0 * min(times[v]), 1000.0 * max(times[v])]
            results[(name, what)] = rec
            print(json.dumps(rec))
    cols = [v for v, _, _ in variants]
    print('\n| batch | forward: ' + ' | forward: '.join(cols) + ' | loss+bwd: ' + ' | loss+bwd: '.join(cols) + ' |')
    print('|---|' + '---:|' * (2 * len(cols)))
    for name in work:
        row = ['%.0f' % results[(name, what)][v + '_us'] for what in ('forward', 'loss_bwd') for v in cols]
        print('| %s | %s |' % (name, ' | '.join(row)))


if __name__ == '__main__':
    main()
