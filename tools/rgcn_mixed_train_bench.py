"""Training the R-GCN model on windows of one query type whatever the formulas: RGCNEncoderDecoder.margin_loss_ids_mixed
+ backward() (one mpqe_rgcn_fwd_mixed_save and one mpqe_rgcn_bwd_mixed per window) against margin_loss_ids_by_runs +
backward() (the module path: one forward and backward of the per-op kernels per run of equal formula) on the SAME windows
and negatives. Needs a GPU (it fails without one: there is no other path).

Per KG and query type: a window of --window queries drawn from kg.MixedQuerySet (sample_query_sets(batched=True)), its
positions sorted; the two sides alternate round by round in one process, every round closed by a device synchronise,
after every shape was warmed up. Before timing, loss and gradients of the two sides are compared at the timed size as
tests/test_rgcn_mixed_train_gpu.py compares them (loss within FWD, gradients within BWD of tests/gqe_oracle.py).

    python tools/rgcn_mixed_train_bench.py [--kgs small aifb] [--embed-dim 128] [--window 512] [--rounds 20]
        [--readout mp] [--out profiles/rgcn_mixed_train_bench.json]

One JSON row per (kg, query type): formulas and runs in the window, min / median / max ms of both sides."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

QUERY_TYPES = ['1-chain', '2-chain', '3-chain', '2-inter', '3-inter', '3-inter_chain', '3-chain_inter']
SHAPES = {'small': (480, 4, 8)}
FWD = dict(rtol=1e-5, atol=1e-6)           # tests/gqe_oracle.py
BWD = dict(rtol=1e-4, atol=2e-6)


def build(kg, args, device):
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.kg import KGIndex, MixedQuerySet
    from mpqe_amd.model import RGCNEncoderDecoder
    schema = synthetic.make_schema(*(SHAPES.get(kg) or synthetic.KG_SHAPES[kg]), seed=args.seed)
    adj = synthetic.make_adjacency(schema, degree=args.degree, seed=args.seed)
    torch.manual_seed(args.seed)
    graph = synthetic.SchemaGraph(schema, args.embed_dim)
    graph.adj_lists = adj
    fm, node_maps = make_feature_modules(schema.ids, args.embed_dim, schema.num_entities)
    model = RGCNEncoderDecoder(graph, DirectEncoder(None, fm, node_maps), readout=args.readout, num_layers=3,
                               shared_layers=False, adaptive=True, weight_decay=0).to(device)
    index = KGIndex.from_graph(graph, node_maps, device)
    sets = index.sample_query_sets(QUERY_TYPES, args.per_type, args.seed + 2, neg_sample_max=args.neg_max, batched=True)
    index.check()
    return model, MixedQuerySet.from_sets(sets)


def stats(ms):
    return dict(min=float(np.min(ms)), median=float(np.median(ms)), max=float(np.max(ms)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--kgs', nargs='+', default=['small', 'aifb'])
    ap.add_argument('--embed-dim', type=int, default=128)
    ap.add_argument('--window', type=int, default=512)
    ap.add_argument('--per-type', type=int, default=2048)
    ap.add_argument('--neg-max', type=int, default=20)
    ap.add_argument('--degree', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--readout', default='mp', choices=['mp', 'sum', 'max'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('rgcn_mixed_train_bench: needs a GPU')
    from mpqe_amd.model import formula_runs, margin_loss_ids_by_runs
    device = torch.device('cuda:0')
    rows = []
    for kg in args.kgs:
        model, mixed = build(kg, args, device)
        gen = torch.Generator().manual_seed(args.seed + 5)
        windows, sides = {}, {}
        for k, (qt, ms) in enumerate(mixed.items()):
            idx = torch.sort(torch.randint(len(ms), (args.window,), generator=gen, dtype=torch.long)).values.to(device)
            sampler = ms.negative_sampler()
            neg = sampler.sample(idx, 100 + k, hard_negatives='inter' in qt)
            sampler.check()
            windows[qt] = (ms,) + ms.take(idx) + (neg,)

        def one(qt, mixed_side):
            ms, fo, anchors, targets, neg = windows[qt]
            model.zero_grad(set_to_none=True)
            if mixed_side:
                loss = model.margin_loss_ids_mixed(ms.formulas, fo, anchors, targets, neg)
            else:
                loss = margin_loss_ids_by_runs(model, ms.formulas, fo, anchors, targets, neg)
            loss.backward()
            return loss

        # agreement at the timed size, which also warms every shape up
        for qt in windows:
            got = {}
            for side in (True, False):
                loss = one(qt, side)
                got[side] = (loss.detach().cpu().numpy(), {k: None if p.grad is None else p.grad.detach().cpu().numpy()
                                                           for k, p in model.named_parameters()})
            np.testing.assert_allclose(got[True][0], got[False][0], **FWD)
            for k, w in got[False][1].items():
                g = got[True][1][k]
                if w is None:
                    assert g is None or not g.any(), k
                else:
                    np.testing.assert_allclose(g, w, err_msg=k, **BWD)
            for _ in range(args.warmup):
                one(qt, True)
                one(qt, False)
        torch.cuda.synchronize()
        times = {(qt, side): [] for qt in windows for side in (True, False)}
        for _ in range(max(args.rounds, 20)):
            for qt in windows:
                for side in (True, False):
                    t0 = time.perf_counter()
                    one(qt, side)
                    torch.cuda.synchronize()
                    times[(qt, side)].append(1e3 * (time.perf_counter() - t0))
        for qt, (ms, fo, anchors, targets, neg) in windows.items():
            fo_host = fo.cpu().numpy()
            row = dict(kg=kg, query_type=qt, readout=args.readout, embed_dim=args.embed_dim, window=args.window, set_queries=len(ms),
                       set_formulas=len(ms.formulas), window_formulas=int(np.unique(fo_host).shape[0]),
                       window_runs=len(formula_runs(fo_host)), rounds=max(args.rounds, 20),
                       mixed_ms=stats(times[(qt, True)]), runs_ms=stats(times[(qt, False)]))
            row['mixed_slowest_below_runs_fastest'] = row['mixed_ms']['max'] < row['runs_ms']['min']
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)
    return rows


if __name__ == '__main__':
    main()
