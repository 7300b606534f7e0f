"""End-task run on a synthetic KG with a REAL adjacency: the reference's training loop (train_helpers.py:76-120: per
step one 1-chain batch + path_weight x {2,3}-chain + inter_weight x (normal + hard-negative batch of each intersection
type), loss.backward(), Adam; evaluation by ROC-AUC with one sampled negative per query, utils.py:34-69) through

  * the product path: FusedTrainStep (one C-ABI call per step) + FlatOptimizer(adam) + NegativeSampler (device draws) +
    mpqe_amd.evaluation.eval_auc_queries on the drop-in modules, and
  * (--oracle) the CPU oracle in the reference's op sequence + torch.optim.Adam on the SAME schedule: same formulas, same
    query indices, same negatives (the sampler's counter-based stream is reproduced on the CPU bit for bit).

    python tools/train_synthetic.py --kg aifb --embed-dim 128 --batch-size 512 --steps 300            # GPU only
    python tools/train_synthetic.py --kg small --embed-dim 64 --batch-size 64 --steps 300 --oracle    # both, compared
    python tools/train_synthetic.py --model gqe --kg small --embed-dim 64 --batch-size 64 --steps 300 # the GQE baseline
    python tools/train_synthetic.py --model gqe --kg small --steps 300 --kg-index    # its filtered metrics through kg.KGIndex
    python tools/train_synthetic.py --model gqe --kg small --steps 300 --device-queries   # queries sampled on the device index
    python tools/train_synthetic.py --model gqe --kg small --steps 300 --device-queries --device-eval   # ... and scored there
    python tools/train_synthetic.py --model gqe --kg small --steps 300 --device-queries --device-eval --mixed-eval   # ... by query type
    python tools/train_synthetic.py --model gqe --kg small --steps 300 --device-queries --device-rank   # filtered MRR / hits@10 on the device sets
    python tools/train_synthetic.py --model gqe --kg small --steps 300 --device-queries --device-eval --mixed-eval --device-rank   # ... one ranking call a window
    python tools/train_synthetic.py --model gqe --kg small --steps 100 --depth 1 --kg-index    # the neighbourhood encoder, on the index
    python tools/train_synthetic.py --kg small --steps 100 --depth 2 --kg-index                 # ... two layers, under the R-GCN model

Prints one JSON line: loss curves, AUC before / after training on held-out queries of the same KG (both sides).
Only tests/ and this tool's --oracle leg use oracle/ (the checker, never the thing trained or shipped).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATH_WEIGHT, INTER_WEIGHT = 0.01, 0.005          # reference train_helpers.py:60-61 (defaults of run_train)
KG_EXTRA = {'small': (480, 4, 8)}


def build(args, device):
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.model import RGCNEncoderDecoder
    shape = KG_EXTRA.get(args.kg) or synthetic.KG_SHAPES[args.kg]
    schema = synthetic.make_schema(*shape, seed=args.seed)
    adj = synthetic.make_adjacency(schema, degree=args.degree, seed=args.seed)
    torch.manual_seed(args.seed)
    graph = synthetic.SchemaGraph(schema, args.embed_dim)
    fm, node_maps = make_feature_modules(schema.ids, args.embed_dim, schema.num_entities)
    model = RGCNEncoderDecoder(graph, DirectEncoder(None, fm, node_maps), readout=args.readout, num_layers=3,
                               shared_layers=False, adaptive=args.readout == 'mp', weight_decay=0)
    rng = np.random.RandomState(args.seed + 1)
    train, test = {}, {}
    if getattr(args, 'device_queries', False):
        train, test = device_queries(args, schema, adj, node_maps, device)
        return schema, graph, node_maps, model, train, test
    for qt in sorted(set(q for q, _ in synthetic.FULL_MIX)):
        train[qt], test[qt] = [], []
        for _ in range(args.formulas):
            f = synthetic.sample_formula(schema, qt, rng)
            train[qt].append((f, synthetic.sample_grounded_queries(schema, adj, f, args.train_queries, rng)))
            test[qt].append((f, synthetic.sample_grounded_queries(schema, adj, f, args.test_queries, rng)))
    return schema, graph, node_maps, model, train, test


def device_queries(args, schema, adj, node_maps, device):
    """--device-queries: the train / test sets through kg.KGIndex.sample_query_sets (the reference's Graph.sample_queries /
    sample_test_queries on the device) instead of synthetic.sample_grounded_queries. A tenth of the edges is held out: the
    training queries are walked on the rest, the test queries on the whole graph and kept only where the target does not
    answer them on the training graph. The formulas are the ones the walk meets, --formulas x --train-queries /
    --test-queries queries per type in all. args.query_sets keeps the training QuerySets (their device samplers)."""
    from mpqe_amd import synthetic
    from mpqe_amd.graph import reverse_relation
    from mpqe_amd.kg import KGIndex
    rng = np.random.RandomState(args.seed + 3)
    full, kept = {}, {}
    for rel in adj:
        if rel in full:
            continue
        inv = reverse_relation(rel)
        pairs = np.array([(n, d) for n in sorted(adj[rel]) for d in sorted(adj[rel][n])], dtype=np.int64).reshape(-1, 2)
        keep = rng.rand(pairs.shape[0]) >= 0.1
        full[rel], full[inv] = (pairs[:, 0], pairs[:, 1]), (pairs[:, 1], pairs[:, 0])
        kept[rel], kept[inv] = (pairs[keep, 0], pairs[keep, 1]), (pairs[keep, 1], pairs[keep, 0])
    index = KGIndex.from_edges(schema, full, node_maps, device)
    train_index = KGIndex.from_edges(schema, kept, node_maps, device)
    types = sorted(set(q for q, _ in synthetic.FULL_MIX))
    t0 = time.perf_counter()
    batched = bool(getattr(args, 'batched_queries', False))
    train_sets = train_index.sample_query_sets(types, args.formulas * args.train_queries, args.seed + 1, batched=batched)
    test_sets = index.sample_query_sets(types, args.formulas * args.test_queries, args.seed + 2, train_index=train_index,
                                        max_rounds=32, batched=batched)
    index.check()
    train_index.check()
    torch.cuda.synchronize()
    args.query_sets, args.sampling_seconds = {}, time.perf_counter() - t0
    args.train_sets = train_sets
    train, test = {qt: [] for qt in types}, {qt: [] for qt in types}
    for f, qs in train_sets.items():
        args.query_sets[(f.query_type, len(train[f.query_type]))] = qs
        train[f.query_type].append((f, qs.queries()))
    args.test_sets = test_sets
    for f, qs in test_sets.items():
        test[f.query_type].append((f, qs.queries()))
    args.sampled = {'train_queries': sum(len(q) for v in train.values() for _, q in v),
                    'test_queries': sum(len(q) for v in test.values() for _, q in v),
                    'train_formulas': len(train_sets), 'test_formulas': len(test_sets), 'seconds': args.sampling_seconds}
    missing = [qt for qt in types if not train[qt] or not test[qt]]
    if missing:
        raise RuntimeError('--device-queries: no query of %s found on this graph' % missing)
    return train, test


def schedule(args, train):
    """Per step the 11 batches of the post-burn-in mix: (query type, hard, formula index, query positions, seed, weight)."""
    from mpqe_amd import synthetic
    rng = np.random.RandomState(args.seed + 2)
    steps = []
    for it in range(args.steps):
        row = []
        for k, (qt, hard) in enumerate(synthetic.FULL_MIX):
            fi = int(rng.randint(len(train[qt])))
            idx = rng.randint(len(train[qt][fi][1]), size=args.batch_size).astype(np.int64)
            w = 1.0 if qt == '1-chain' else (INTER_WEIGHT if 'inter' in qt else PATH_WEIGHT)
            row.append((qt, hard, fi, idx, 100000 * (it + 1) + k, w * args.weight_scale if qt != '1-chain' else w))
        steps.append(row)
    return steps


def test_dict(test):
    out = {}
    for qt in test:
        for f, qs in test[qt]:
            out.setdefault(f, []).extend(qs)
    return out


def model_queries(args, tq):
    """What the model's evaluation takes: the test QuerySets themselves under --device-eval (evaluation.eval_*_queries then
    score and rank on the device: no Query object, no id list, no score on the host), else the lists of Query."""
    return eval_sets(args) if getattr(args, 'device_eval', False) else tq


def eval_sets(args):
    """the test QuerySets, or under --mixed-eval the same sets grouped by query type (kg.MixedQuerySet.from_sets, once)"""
    if not getattr(args, 'mixed_eval', False):
        return args.test_sets
    if getattr(args, 'test_mixed', None) is None:
        from mpqe_amd.kg import MixedQuerySet
        args.test_mixed = MixedQuerySet.from_sets(args.test_sets)
    return args.test_mixed


def rank_queries(args, tq, known):
    """What eval_rank_queries takes as (queries, known_answers): under --device-rank the test QuerySets (grouped by query
    type under --mixed-eval) and the index they were sampled on -- ranked on the device, the answers computed there --, else
    the lists of Query and the caller's known answers."""
    if not getattr(args, 'device_rank', False):
        return tq, known
    return eval_sets(args), next(iter(args.test_sets.values())).index


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--kg', default='small')
    ap.add_argument('--embed-dim', type=int, default=64)
    ap.add_argument('--batch-size', type=int, default=64)
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--lr', type=float, default=0.01)
    ap.add_argument('--readout', default='mp')
    ap.add_argument('--degree', type=int, default=2)
    ap.add_argument('--formulas', type=int, default=2, help='formulas per query type')
    ap.add_argument('--train-queries', type=int, default=256, help='per formula')
    ap.add_argument('--test-queries', type=int, default=96, help='per formula')
    ap.add_argument('--weight-scale', type=float, default=1.0,
                    help='multiplies the reference path / inter weights (0.01 / 0.005): 100 makes every batch type count')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--oracle', action='store_true', help='also train through the CPU oracle + torch.optim.Adam and compare')
    ap.add_argument('--eval-every', type=int, default=0)
    ap.add_argument('--dropin', action='store_true',
                    help="train through the reference's own loop body and entry points (model.margin_loss, loss.backward(): "
                         'mpqe_amd/dropin.py) instead of FusedTrainStep.pack / run')
    ap.add_argument('--model', default='rgcn', choices=['rgcn', 'gqe'],
                    help="gqe: the baseline QueryEncoderDecoder (the reference's --model gqe) through the reference's loop body")
    ap.add_argument('--decoder', default='bilinear', choices=['bilinear', 'transe', 'bilinear-diag'],
                    help='gqe: metapath decoder (the reference\'s --decoder)')
    ap.add_argument('--inter-decoder', default='mean', help='gqe: mean | min | mean-simple | min-simple (--inter_decoder)')
    ap.add_argument('--kg-index', action='store_true',
                    help='gqe: the filtered metrics take their known answers from the device index (mpqe_amd/kg.py) instead of '
                         'the host walk over the adjacency: same numbers')
    ap.add_argument('--device-queries', action='store_true',
                    help='sample the train / test queries and their negatives on the device index (kg.KGIndex.sample_query_sets: '
                         'the reference\'s KG sampler) instead of the host stand-in synthetic.sample_grounded_queries')
    ap.add_argument('--batched-queries', action='store_true',
                    help='with --device-queries: sample_query_sets(batched=True) -- queries of different formulas answered in one '
                         'launch per query type, the same queries per formula; the draws below the cap of 100 negatives differ')
    ap.add_argument('--device-eval', action='store_true',
                    help='with --device-queries: evaluate the model on the test QuerySets themselves (AUC and percentile rank '
                         'computed on the device, evaluation.eval_auc_queries / eval_perc_queries over kg.QuerySet); the '
                         'sampled negatives then come from the library\'s stream, not Python\'s')
    ap.add_argument('--mixed-eval', action='store_true',
                    help='with --device-eval: group the test sets by query type (kg.MixedQuerySet) and score queries of '
                         'different formulas per call -- one launch a window under --model gqe; other sampled negatives')
    ap.add_argument('--device-rank', action='store_true',
                    help='with --device-queries: the filtered ranking metrics over the test QuerySets themselves '
                         '(evaluation.eval_rank_queries on the device route, known answers from the sets\' index); with '
                         '--mixed-eval over kg.MixedQuerySets: one ranking call a window whatever the formulas')
    ap.add_argument('--mixed-train', action='store_true',
                    help='with --device-queries: train on windows of one query type whatever the formulas '
                         '(kg.MixedQuerySet.take + the model\'s margin_loss_ids_mixed: one mixed forward and one mixed '
                         'backward per window, under either --model) instead of one formula per batch')
    ap.add_argument('--depth', type=int, default=0, choices=[0, 1, 2],
                    help='entity encoder (the reference\'s --depth): 0 the embedding lookup (everything above), 1 / 2 the '
                         'neighbourhood-aggregating Encoder of utils.get_encoder under either --model, trained through '
                         'model.margin_loss; on the device index with --kg-index or --device-queries, else the host path')
    args = ap.parse_args(argv)
    if args.batched_queries and not args.device_queries:
        ap.error('--batched-queries needs --device-queries')
    if args.device_eval and (not args.device_queries or args.depth):
        ap.error('--device-eval needs --device-queries and the embedding-lookup encoder (--depth 0)')
    if args.device_rank and (not args.device_queries or args.depth):
        ap.error('--device-rank needs --device-queries and the embedding-lookup encoder (--depth 0)')
    if args.mixed_eval and not args.device_eval:
        ap.error('--mixed-eval needs --device-eval')
    if args.mixed_train and (not args.device_queries or args.depth or
                             (args.model == 'rgcn' and args.readout not in ('mp', 'sum', 'max'))):
        ap.error('--mixed-train needs --device-queries and the embedding-lookup encoder (--depth 0); under --model rgcn a '
                 'readout without parameters (mp | sum | max)')
    if args.mixed_train and args.dropin:
        ap.error('--mixed-train and --dropin are two different loops: choose one')
    if args.depth:
        out = run_depth(args)
    elif args.model == 'gqe':
        out = run_gqe(args)
    elif args.mixed_train:
        out = run_rgcn_mixed(args)
    else:
        out = run_dropin(args) if args.dropin else run(args)
    if getattr(args, 'device_queries', False):
        out['device_queries'] = args.sampled
    print(json.dumps(out))
    return out


def run(args):
    from mpqe_amd import evaluation
    from mpqe_amd.fused import FusedTrainStep
    from mpqe_amd.optim import FlatOptimizer
    from mpqe_amd.sampling import NegativeSampler
    device = torch.device('cuda:0')
    schema, graph, node_maps, model, train, test = build(args, device)
    cpu_state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(device)
    steps = schedule(args, train)
    tq = test_dict(test)
    samplers = {}
    for qt in train:
        for fi, (f, qs) in enumerate(train[qt]):
            if getattr(args, 'device_queries', False):
                samplers[(qt, fi)] = args.query_sets[(qt, fi)].negative_sampler()         # the sampled CSRs, on the device
                continue
            samplers[(qt, fi)] = NegativeSampler(qs, device, full_list=graph.full_lists[f.target_mode] if qt == '1-chain' else None)
    anchors = {(qt, fi): np.array([q.anchor_nodes for q in qs], dtype=np.int64) for qt in train for fi, (f, qs) in enumerate(train[qt])}
    targets = {(qt, fi): np.array([q.target_node for q in qs], dtype=np.int64) for qt in train for fi, (f, qs) in enumerate(train[qt])}

    fstep = FusedTrainStep(model)
    opt = FlatOptimizer(fstep, lr=args.lr, opt='adam')
    with torch.no_grad():
        auc0, _ = evaluation.eval_auc_queries(model_queries(args, tq), model, batch_size=128, seed=0)
    losses, negs_used, aucs = [], [], []
    t0 = time.perf_counter()
    for it, row in enumerate(steps):
        batches, negs_row = [], []
        for qt, hard, fi, idx, seed, w in row:
            f = train[qt][fi][0]
            neg = samplers[(qt, fi)].sample(idx, seed, hard_negatives=hard).cpu().numpy()
            negs_row.append(neg)
            batches.append(dict(formula=f, anchor_ids=anchors[(qt, fi)][idx], targets=targets[(qt, fi)][idx], negs=neg, weight=w))
        packed = fstep.pack(batches)
        assert fstep.uses_chain(packed) or model.emb_dim not in (64, 128, 256)
        loss = fstep.run(packed)
        opt.step()
        losses.append(loss)
        negs_used.append(negs_row)
        if args.eval_every and (it + 1) % args.eval_every == 0:
            with torch.no_grad():
                aucs.append((it + 1, evaluation.eval_auc_queries(model_queries(args, tq), model, batch_size=128, seed=0)[0]))
    fstep.check()
    for s in samplers.values():
        s.check()
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    losses = torch.stack(losses).cpu().numpy()            # [steps, 1 + 11]
    with torch.no_grad():
        auc1, per1 = evaluation.eval_auc_queries(model_queries(args, tq), model, batch_size=128, seed=0)
    out = dict(kg=args.kg, embed_dim=args.embed_dim, batch_size=args.batch_size, steps=args.steps, readout=args.readout,
               chain_form=bool(fstep.uses_chain(packed)), train_seconds=train_s,
               loss_first=float(losses[0, 0]), loss_last20=float(losses[-20:, 0].mean()), auc_before=float(auc0),
               auc_after=float(auc1), auc_curve=aucs, loss_curve=[float(v) for v in losses[:, 0]])
    if getattr(args, 'device_eval', False):
        with torch.no_grad():
            out['perc_after'] = float(evaluation.eval_perc_queries(eval_sets(args), model, batch_size=128))
    if args.oracle:
        out.update(run_oracle(args, graph, node_maps, model, cpu_state, train, tq, steps, negs_used, anchors, targets))
    return out


def run_oracle(args, graph, node_maps, model, cpu_state, train, tq, steps, negs_used, anchors, targets):
    """The same schedule through the CPU oracle (reference op sequence, two encoder passes) + torch.optim.Adam."""
    from mpqe_amd import evaluation
    from oracle import ref_cpu            # the checker
    params = {k: v.clone().requires_grad_(True) for k, v in cpu_state.items()}
    cfg = dict(readout=args.readout, scatter_op='add', num_layers=3, adaptive=args.readout == 'mp', weight_decay=0)
    node_map = node_maps.cpu() if torch.is_tensor(node_maps) else node_maps
    opt = torch.optim.Adam(list(params.values()), lr=args.lr)
    # the reference's era (torch 1.4) zeroes gradients in place: a parameter that has had a gradient once keeps being
    # updated (zero gradient: its moments decay, its momentum moves it). The flat optimiser is dense Adam over every
    # parameter from step 1 -- the same thing when every parameter TENSOR is touched in the first step, which the
    # 11-batch mix does; the zero gradients are materialised here so that both sides are that rule exactly.
    for p in params.values():
        p.grad = torch.zeros_like(p)

    class Q(object):
        def __init__(self, a):
            self.anchor_nodes = tuple(int(v) for v in a)

    class Oracle(object):
        def forward(self, formula, queries, tg, neg_nodes=None, neg_lengths=None):
            col = ref_cpu.collate(formula, queries, model.rel_ids, model.mode_ids)
            return ref_cpu.forward(params, cfg, node_map, formula, col, tg, neg_nodes, neg_lengths)
    with torch.no_grad():
        auc0, _ = evaluation.eval_auc_queries(tq, Oracle(), batch_size=128, seed=0)
    losses = []
    t0 = time.perf_counter()
    for it, row in enumerate(steps):
        opt.zero_grad(set_to_none=False)
        total = 0
        for k, (qt, hard, fi, idx, seed, w) in enumerate(row):
            f, qs = train[qt][fi]
            # (the device sampler's draws, reproduced by the oracle's CPU stream: tests/test_fused_gpu.py checks the equality)
            col = ref_cpu.collate(f, [Q(a) for a in anchors[(qt, fi)][idx]], model.rel_ids, model.mode_ids)
            l = ref_cpu.margin_loss(params, cfg, node_map, f, col, targets[(qt, fi)][idx], negs_used[it][k])
            total = total + w * l
        total.backward()
        opt.step()
        losses.append(float(total.item()))
    with torch.no_grad():
        auc1, _ = evaluation.eval_auc_queries(tq, Oracle(), batch_size=128, seed=0)
    return dict(oracle_seconds=time.perf_counter() - t0, oracle_loss_first=losses[0],
                oracle_loss_last20=float(np.mean(losses[-20:])), oracle_auc_before=float(auc0), oracle_auc_after=float(auc1),
                oracle_loss_curve=losses)


def _reference_loop(model_like, iterators, query_types, optimizer, steps, margin_loss):
    """The body of the reference's run_train (train_helpers.py:76-120, post-burn-in phase), verbatim in structure:
    margin_loss(batch) per query type, `loss += w * ...`, loss.item(), backward, optimizer step. -> the losses."""
    losses = []
    for _ in range(steps):
        optimizer.zero_grad()
        loss = margin_loss(next(iterators['1-chain']), False)
        for qt in query_types:
            if qt == '1-chain':
                continue
            if 'inter' in qt:
                loss += INTER_WEIGHT * margin_loss(next(iterators[qt]), False)
                loss += INTER_WEIGHT * margin_loss(next(iterators[qt]), True)
            else:
                loss += PATH_WEIGHT * margin_loss(next(iterators[qt]), False)
        losses.append(loss.item())
        loss.backward()
        optimizer.step()
    return losses


def run_dropin(args):
    """End-task run through the reference's OWN entry points (mpqe_amd/dropin.py): the run_train loop body over
    get_queries_iterator batches, model.margin_loss with python's random negatives, loss.backward(), FlatOptimizer --
    beside the same loop through the CPU oracle + torch.optim.Adam. Both sides seed numpy (formula draws) and python's
    `random` (negative draws) alike, and the drop-in replays python's stream exactly, so the two runs see the SAME batches
    and the SAME negatives without any of them being recorded."""
    import random
    from mpqe_amd import evaluation
    from mpqe_amd.data_utils import get_queries_iterator
    from mpqe_amd.optim import FlatOptimizer
    from oracle import ref_cpu            # the checker
    device = torch.device('cuda:0')
    schema, graph, node_maps, model, train, test = build(args, device)
    graph.full_lists = {m: [int(v) for v in ids] for m, ids in graph.full_lists.items()}
    cpu_state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(device)
    tq = test_dict(test)
    by_type = {qt: {f: qs for f, qs in train[qt]} for qt in train}
    order = [qt for qt, _ in __import__('mpqe_amd.synthetic', fromlist=['FULL_MIX']).FULL_MIX]
    query_types = list(dict.fromkeys(order))

    def iterators(m):
        np.random.seed(args.seed + 11)
        return {qt: get_queries_iterator(by_type[qt], args.batch_size, m) for qt in by_type}
    # ---- the product path
    with torch.no_grad():
        auc0, _ = evaluation.eval_auc_queries(model_queries(args, tq), model, batch_size=128, seed=0)
    assert model.dropin() is not None, 'the model did not take the fused step'
    opt = FlatOptimizer(model.dropin().step, lr=args.lr, opt='adam')
    random.seed(args.seed + 12)
    t0 = time.perf_counter()
    losses = _reference_loop(model, iterators(model), query_types, opt, args.steps,
                             lambda batch, hard: model.margin_loss(*batch, hard_negatives=hard))
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    model.dropin()._check_mirror()
    with torch.no_grad():
        auc1, _ = evaluation.eval_auc_queries(model_queries(args, tq), model, batch_size=128, seed=0)
    out = dict(kg=args.kg, embed_dim=args.embed_dim, batch_size=args.batch_size, steps=args.steps, readout=args.readout,
               train_seconds=train_s, fused_backward_steps=model.dropin().steps, node_impl=model.dropin().node_impl,
               loss_first=losses[0], loss_last20=float(np.mean(losses[-20:])), auc_before=float(auc0), auc_after=float(auc1),
               loss_curve=losses)
    if not args.oracle:
        return out
    # ---- the same loop through the oracle
    params = {k: v.clone().requires_grad_(True) for k, v in cpu_state.items()}
    cfg = dict(readout=args.readout, scatter_op='add', num_layers=3, adaptive=args.readout == 'mp', weight_decay=0)
    node_map = node_maps.cpu() if torch.is_tensor(node_maps) else node_maps
    oopt = torch.optim.Adam(list(params.values()), lr=args.lr)
    for p in params.values():               # (dense Adam over every parameter from step 1: see run_oracle)
        p.grad = torch.zeros_like(p)

    class ZeroInPlace(object):
        def zero_grad(self):
            oopt.zero_grad(set_to_none=False)

        def step(self):
            oopt.step()

    def oracle_margin_loss(batch, hard):
        formula, queries = batch[0], batch[1]
        if hard:                                                        # reference model.py:470-476, literally
            negs = [random.choice(q.hard_neg_samples) for q in queries]
        elif formula.query_type == '1-chain':
            negs = [random.choice(graph.full_lists[formula.target_mode]) for _ in queries]
        else:
            negs = [random.choice(q.neg_samples) for q in queries]
        col = ref_cpu.collate(formula, queries, model.rel_ids, model.mode_ids)
        return ref_cpu.margin_loss(params, cfg, node_map, formula, col, np.array([q.target_node for q in queries]), np.array(negs))

    class Oracle(object):
        def forward(self, formula, queries, tg, neg_nodes=None, neg_lengths=None):
            col = ref_cpu.collate(formula, queries, model.rel_ids, model.mode_ids)
            return ref_cpu.forward(params, cfg, node_map, formula, col, tg, neg_nodes, neg_lengths)
    with torch.no_grad():
        oauc0, _ = evaluation.eval_auc_queries(tq, Oracle(), batch_size=128, seed=0)
    random.seed(args.seed + 12)
    t0 = time.perf_counter()
    olosses = _reference_loop(None, iterators(model), query_types, ZeroInPlace(), args.steps, oracle_margin_loss)
    with torch.no_grad():
        oauc1, _ = evaluation.eval_auc_queries(tq, Oracle(), batch_size=128, seed=0)
    out.update(oracle_seconds=time.perf_counter() - t0, oracle_loss_first=olosses[0], oracle_loss_last20=float(np.mean(olosses[-20:])),
               oracle_auc_before=float(oauc0), oracle_auc_after=float(oauc1), oracle_loss_curve=olosses)
    return out


def build_gqe(args, device):
    """build() with the GQE baseline in the R-GCN model's place: the same KG, entity tables and queries."""
    from mpqe_amd.model import QueryEncoderDecoder
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    schema, graph, node_maps, rgcn, train, test = build(args, device)
    graph.full_lists = {m: [int(v) for v in ids] for m, ids in graph.full_lists.items()}
    dims = {m: args.embed_dim for m in schema.modes}
    torch.manual_seed(args.seed)
    model = QueryEncoderDecoder(graph, rgcn.enc, get_metapath_decoder(graph, dims, args.decoder, vector_decoders=True),
                                get_intersection_decoder(graph, dims, args.inter_decoder)).to(device)
    return schema, graph, node_maps, model, train, test


def known_answers(args, schema, tq):
    """{query: every entity the KG's adjacency gives as an answer}: what the filtered ranking metrics exclude."""
    from mpqe_amd import synthetic
    adj = synthetic.make_adjacency(schema, degree=args.degree, seed=args.seed)
    return {q: synthetic._answers(adj, f, list(q.anchor_nodes))[0] for f in tq for q in tq[f]}


def kg_index(args, schema, node_maps, device):
    """The same adjacency as a kg.KGIndex on the device: eval_rank_queries(known_answers=index) answers each batch there."""
    from mpqe_amd import synthetic
    from mpqe_amd.kg import KGIndex
    adj = synthetic.make_adjacency(schema, degree=args.degree, seed=args.seed)
    edges = {}
    for rel, lists in adj.items():
        lens = np.fromiter((len(s) for s in lists.values()), dtype=np.int64, count=len(lists))
        edges[rel] = (np.repeat(np.fromiter(lists.keys(), dtype=np.int64, count=len(lists)), lens),
                      np.fromiter((d for s in lists.values() for d in s), dtype=np.int64, count=int(lens.sum())))
    return KGIndex.from_edges(schema, edges, node_maps, device)


def mixed_windows(args, model, query_types, device):
    """--mixed-train: a batch is batch_size positions of a query type's concatenation, whatever their formulas; sorted, so
    that equal formulas sit next to each other (longer stretches, fewer matrix reads). -> (the iterators and the
    margin_loss of _reference_loop, the negative samplers): kg.MixedQuerySet.take + model.margin_loss_ids_mixed."""
    from mpqe_amd.kg import MixedQuerySet
    mixed = MixedQuerySet.from_sets(args.train_sets)
    samplers = {qt: ms.negative_sampler() for qt, ms in mixed.items()}
    gen = torch.Generator().manual_seed(args.seed + 13)
    draws = [0]

    def positions(qt):
        while True:
            idx = torch.randint(len(mixed[qt]), (args.batch_size,), generator=gen, dtype=torch.long)
            yield qt, torch.sort(idx).values.to(device)

    def margin_loss(batch, hard):
        qt, idx = batch
        ms = mixed[qt]
        draws[0] += 1
        neg = samplers[qt].sample(idx, args.seed + 100000 + draws[0], hard_negatives=hard)
        formula_of, anchors, targets = ms.take(idx)
        return model.margin_loss_ids_mixed(ms.formulas, formula_of, anchors, targets, neg)
    return {qt: positions(qt) for qt in query_types}, margin_loss, samplers


def run_rgcn_mixed(args):
    """--mixed-train under --model rgcn: the R-GCN model (embedding-lookup encoder, a readout without parameters) through
    the reference's loop body on mixed windows -- RGCNEncoderDecoder.margin_loss_ids_mixed: one mixed forward with states
    and one mixed backward per window --, loss.backward(), Adam; ROC-AUC before and after."""
    import random
    from mpqe_amd import evaluation, optim
    device = torch.device('cuda:0')
    schema, graph, node_maps, model, train, test = build(args, device)
    model = model.to(device)
    tq = test_dict(test)
    order = [qt for qt, _ in __import__('mpqe_amd.synthetic', fromlist=['FULL_MIX']).FULL_MIX]
    query_types = list(dict.fromkeys(order))
    iterators, margin_loss, samplers = mixed_windows(args, model, query_types, device)
    with torch.no_grad():
        auc0, _ = evaluation.eval_auc_queries(model_queries(args, tq), model, batch_size=128, seed=0)
    opt = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=args.lr)
    random.seed(args.seed + 12)
    t0 = time.perf_counter()
    losses = _reference_loop(model, iterators, query_types, opt, args.steps, margin_loss)
    for sampler in samplers.values():
        sampler.check()
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    with torch.no_grad():
        auc1, _ = evaluation.eval_auc_queries(model_queries(args, tq), model, batch_size=128, seed=0)
    out = dict(model='rgcn', kg=args.kg, embed_dim=args.embed_dim, batch_size=args.batch_size, steps=args.steps,
               readout=args.readout, train_seconds=train_s, loss_first=losses[0], loss_last20=float(np.mean(losses[-20:])),
               auc_before=float(auc0), auc_after=float(auc1), loss_curve=losses, mixed_train=True)
    if getattr(args, 'device_eval', False):
        with torch.no_grad():
            out['perc_after'] = float(evaluation.eval_perc_queries(eval_sets(args), model, batch_size=128))
    return out


def run_gqe(args):
    """The GQE baseline (QueryEncoderDecoder, bilinear paths + set intersection) through the reference's loop body
    (_reference_loop): margin_loss per batch on the fused kernels, loss.backward(), Adam; ROC-AUC and the filtered ranking
    metrics over all entities (evaluation.eval_rank_queries: MRR, hits@10) before and after."""
    import random
    from mpqe_amd import evaluation, optim
    device = torch.device('cuda:0')
    schema, graph, node_maps, model, train, test = build_gqe(args, device)
    tq = test_dict(test)
    known = kg_index(args, schema, node_maps, device) if getattr(args, 'kg_index', False) else known_answers(args, schema, tq)
    order = [qt for qt, _ in __import__('mpqe_amd.synthetic', fromlist=['FULL_MIX']).FULL_MIX]
    query_types = list(dict.fromkeys(order))

    def batches(qt):
        rng = np.random.RandomState(args.seed + 11 + query_types.index(qt))
        pos = [0] * len(train[qt])
        while True:
            fi = int(rng.randint(len(train[qt])))
            f, qs = train[qt][fi]
            lo = pos[fi] % len(qs)
            pos[fi] = lo + args.batch_size
            yield f, qs[lo:lo + args.batch_size]
    iterators = {qt: batches(qt) for qt in query_types}
    margin_loss = lambda batch, hard: model.margin_loss(*batch, hard_negatives=hard)       # noqa: E731
    if getattr(args, 'mixed_train', False):
        iterators, margin_loss, samplers = mixed_windows(args, model, query_types, device)
    with torch.no_grad():
        auc0, _ = evaluation.eval_auc_queries(model_queries(args, tq), model, batch_size=128, seed=0)
    rq, rknown = rank_queries(args, tq, known)
    rank0 = evaluation.eval_rank_queries(rq, model.eval(), batch_size=128, ks=(10,), known_answers=rknown)
    model.train()
    opt = optim.Adam(model.parameters(), lr=args.lr)
    random.seed(args.seed + 12)
    t0 = time.perf_counter()
    losses = _reference_loop(model, iterators, query_types, opt, args.steps, margin_loss)
    if getattr(args, 'mixed_train', False):
        for sampler in samplers.values():
            sampler.check()
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    with torch.no_grad():
        auc1, _ = evaluation.eval_auc_queries(model_queries(args, tq), model, batch_size=128, seed=0)
    rank1 = evaluation.eval_rank_queries(rq, model.eval(), batch_size=128, ks=(10,), known_answers=rknown)
    out = dict(model='gqe', decoder=args.decoder, inter_decoder=args.inter_decoder, kg=args.kg, embed_dim=args.embed_dim,
               batch_size=args.batch_size, steps=args.steps, train_seconds=train_s, loss_first=losses[0],
               loss_last20=float(np.mean(losses[-20:])), auc_before=float(auc0), auc_after=float(auc1),
               filtered_mrr_before=rank0['mrr'], filtered_mrr_after=rank1['mrr'], filtered_hits10_before=rank0['hits@10'],
               filtered_hits10_after=rank1['hits@10'],
               known_answers='device-sets' if getattr(args, 'device_rank', False) else
               'kg-index' if getattr(args, 'kg_index', False) else 'host',
               loss_curve=losses)
    if getattr(args, 'device_eval', False):
        with torch.no_grad():
            out['perc_after'] = float(evaluation.eval_perc_queries(eval_sets(args), model, batch_size=128))
    if getattr(args, 'mixed_train', False):
        out['mixed_train'] = True
    return out


def run_depth(args):
    """--depth 1 | 2: either model on utils.get_encoder's neighbourhood encoder, through the reference's loop body
    (_reference_loop: margin_loss per batch on the models' module / composed paths, loss.backward(), Adam) and ROC-AUC
    before and after. With --kg-index or --device-queries the encoder draws and encodes on the device index
    (Encoder(index=...)); otherwise it walks the Python adjacency (the host path; a node without neighbours and the null
    node then read their table's padding row, which the reference's own closure cannot look up)."""
    import random
    from mpqe_amd import evaluation, optim, synthetic
    from mpqe_amd.model import QueryEncoderDecoder, RGCNEncoderDecoder
    from mpqe_amd.utils import get_encoder, get_intersection_decoder, get_metapath_decoder
    device = torch.device('cuda:0')
    schema, graph, node_maps, plain, train, test = build(args, device)
    graph.full_lists = {m: [int(v) for v in ids] for m, ids in graph.full_lists.items()}
    fm = plain.enc.feature_modules
    on_index = bool(getattr(args, 'kg_index', False) or getattr(args, 'device_queries', False))
    index = kg_index(args, schema, node_maps, device) if on_index else None
    maps_dev = node_maps.to(device)
    if index is None:
        graph.adj_lists = synthetic.make_adjacency(schema, degree=args.degree, seed=args.seed)

        def features(nodes, mode):
            ids = torch.as_tensor(nodes, dtype=torch.long, device=device)
            table = fm[mode]
            return table(torch.where(ids < 0, torch.full_like(ids, table.weight.shape[0] - 1), maps_dev[ids.clamp(min=0)]))
        graph.features = features
    dims = {m: args.embed_dim for m in schema.modes}
    torch.manual_seed(args.seed)
    enc = get_encoder(args.depth, graph, dims, fm, True, node_maps=node_maps, index=index)
    if args.model == 'gqe':
        model = QueryEncoderDecoder(graph, enc, get_metapath_decoder(graph, dims, args.decoder, vector_decoders=True),
                                    get_intersection_decoder(graph, dims, args.inter_decoder))
    else:
        model = RGCNEncoderDecoder(graph, enc, readout=args.readout, num_layers=3, shared_layers=False,
                                   adaptive=args.readout == 'mp', weight_decay=0)
    model = model.to(device)
    tq = test_dict(test)
    order = [qt for qt, _ in synthetic.FULL_MIX]
    query_types = list(dict.fromkeys(order))

    def batches(qt):
        rng = np.random.RandomState(args.seed + 11 + query_types.index(qt))
        pos = [0] * len(train[qt])
        while True:
            fi = int(rng.randint(len(train[qt])))
            f, qs = train[qt][fi]
            lo = pos[fi] % len(qs)
            pos[fi] = lo + args.batch_size
            yield f, qs[lo:lo + args.batch_size]
    iterators = {qt: batches(qt) for qt in query_types}
    with torch.no_grad():
        auc0, _ = evaluation.eval_auc_queries(model_queries(args, tq), model, batch_size=128, seed=0)
    opt = optim.Adam(model.parameters(), lr=args.lr)
    random.seed(args.seed + 12)
    t0 = time.perf_counter()
    losses = _reference_loop(model, iterators, query_types, opt, args.steps,
                             lambda batch, hard: model.margin_loss(*batch, hard_negatives=hard))
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    with torch.no_grad():
        auc1, _ = evaluation.eval_auc_queries(model_queries(args, tq), model, batch_size=128, seed=0)
    return dict(model=args.model, depth=args.depth, encoder_path='kg-index' if on_index else 'host', kg=args.kg,
                embed_dim=args.embed_dim, batch_size=args.batch_size, steps=args.steps, train_seconds=train_s,
                loss_first=losses[0], loss_last20=float(np.mean(losses[-20:])), auc_before=float(auc0), auc_after=float(auc1),
                loss_curve=losses)


if __name__ == '__main__':
    main()
