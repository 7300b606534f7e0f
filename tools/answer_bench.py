"""Time of answering a batch of queries over ALL entities of the target mode -- RGCNEncoderDecoder.answer (k = 10) and
rank_targets, the fused score / count / top-k kernel of csrc/rank.hip -- on KG shapes of synthetic.KG_SHAPES at B = 512,
D = 128, beside what a user could write before it: F.normalize(table) -> q_normalised @ t.T -> torch.topk (the library
GEMM, the [B, N] score matrix materialised), fed the same query embeddings.

Device-event timing: warm-up, then `--blocks` blocks of `--iters` calls, one event pair per block, the median block
reported per call. `kernel_*` rows time ops.rank_entities alone (no encoder, no id translation), which is what the
baseline's three ops compare with; `answer` / `rank_targets` are the whole calls, encoder included.

    python tools/answer_bench.py [--kgs aifb mutag am] [--batch 512] [--dim 128]

--model gqe: the GQE baseline (QueryEncoderDecoder), per query type, three ways to the same answers:
  fused     model.answer (k = 10) / model.rank_targets: ops.gqe_embed + ops.rank_entities, a chain formula's candidates
            projected once (`*_cached`: eval() mode, the projection kept from the call before; plain: train() mode,
            projected in every call)
  torch     the same arithmetic in plain torch ops: F.normalize, matrix products, the [B, n] cosine matrix, torch.topk
  forward   the only route before answer(): model.forward with every entity as a ragged negative of every query (the
            B n scores written to memory; the top-k / rank over them not included)

    python tools/answer_bench.py --model gqe --kgs small aifb --batch 128 --dim 128
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32_MATRIX_TFLOPS = 157.3        # MI355X, v_mfma_f32_32x32x2_f32
KG_EXTRA = {'small': (480, 4, 8)}      # tools/train_synthetic.py's small KG


def timed(fn, warmup, blocks, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def build(kg, dim, seed=0):
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.model import RGCNEncoderDecoder
    schema = synthetic.make_schema(*synthetic.KG_SHAPES[kg], seed=seed)
    torch.manual_seed(seed)
    graph = synthetic.SchemaGraph(schema, dim)
    fm, node_maps = make_feature_modules(schema.ids, dim, schema.num_entities)
    model = RGCNEncoderDecoder(graph, DirectEncoder(None, fm, node_maps), readout='mp', num_layers=3, shared_layers=False,
                               adaptive=True, weight_decay=0)
    return schema, model


def build_gqe(kg, dim, inter, seed=0, decoder='bilinear'):
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.model import QueryEncoderDecoder
    from mpqe_amd.utils import get_intersection_decoder, get_metapath_decoder
    schema = synthetic.make_schema(*(KG_EXTRA.get(kg) or synthetic.KG_SHAPES[kg]), seed=seed)
    torch.manual_seed(seed)
    graph = synthetic.SchemaGraph(schema, dim)
    graph.full_lists = {m: [int(v) for v in ids] for m, ids in graph.full_lists.items()}
    fm, node_maps = make_feature_modules(schema.ids, dim, schema.num_entities)
    dims = {m: dim for m in schema.modes}
    model = QueryEncoderDecoder(graph, DirectEncoder(None, fm, node_maps), get_metapath_decoder(graph, dims, decoder, vector_decoders=True),
                                get_intersection_decoder(graph, dims, inter))
    return schema, model


def gqe_torch_operands(model, formula, queries, n):
    """(q [B, D], candidates [n, D]) of QueryEncoderDecoder.forward's arithmetic in plain torch ops."""
    from mpqe_amd.model import gqe_plan
    form, branches, imode, tail, emode = gqe_plan(formula)
    enc, maps = model.enc, model.enc.node_maps

    def rows(slot, mode):
        ids = torch.as_tensor([q.anchor_nodes[slot] for q in queries], device=maps.device)
        return F.normalize(enc.table(mode)[maps[ids]], dim=1)

    def step(x, rel, transposed):
        dec = model.path_dec
        if hasattr(dec, 'vecs'):
            return x + dec.vecs[rel] if dec.op == 'translate' else x * dec.vecs[rel]
        m = dec.mats[rel]
        return x @ (m.t() if transposed else m)
    if form == 0:
        cand = F.normalize(enc.table(formula.target_mode)[:n], dim=1)
        for rel, t in branches[0][2]:
            cand = step(cand, rel, t)
        return rows(0, formula.anchor_modes[0]), cand
    xs = []
    for slot, mode, steps in branches:
        x = rows(slot, mode)
        for rel, t in steps:
            x = step(x, rel, t)
        xs.append(x)
    pre = getattr(model.inter_dec, 'pre_mats', None)
    if pre is not None:
        xs = [torch.relu(x @ pre[imode].t()) for x in xs]
    st = torch.stack(xs)
    q = st.min(dim=0)[0] if model.inter_dec.agg_kind == 'min' else st.mean(dim=0)
    if pre is not None:
        q = q @ model.inter_dec.post_mats[imode].t()
    for rel, t in tail:
        q = step(q, rel, t)
    return q, enc.table(formula.target_mode)[:n]


def main_gqe(a):
    from mpqe_amd import synthetic
    torch.cuda.set_device(0)
    out = {'tool': 'answer_bench', 'model': 'gqe', 'decoder': a.decoder, 'inter_decoder': a.inter_decoder, 'batch': a.batch, 'dim': a.dim, 'k': a.k,
           'timing': 'device events, median of %d blocks of %d calls after %d warm-up calls' % (a.blocks, a.iters, a.warmup),
           'shapes': {}}
    for kg in a.kgs:
        schema, model = build_gqe(kg, a.dim, a.inter_decoder, decoder=a.decoder)
        model = model.to('cuda:0').eval()
        per_type = {}
        for qt in a.query_types:
            rng = np.random.RandomState(1)
            f = synthetic.sample_formula(schema, qt, rng)
            qs = synthetic.sample_queries(schema, f, a.batch, rng, n_neg=1, n_hard=1)
            ids_all = np.asarray(model.graph.full_lists[f.target_mode], dtype=np.int64)
            n = model._mode_rows(f.target_mode, torch.device('cuda:0'))[0].shape[0]
            targets = [q_.target_node for q_ in qs]
            target_rows = model.enc.node_maps[torch.as_tensor(targets, device='cuda:0')]
            negs, lens = np.tile(ids_all, a.batch).tolist(), [len(ids_all)] * a.batch

            dot = 'inter' not in qt and getattr(model.path_dec, 'score', 'cosine') == 'dot'

            def cosines():
                q, cand = gqe_torch_operands(model, f, qs, n)
                if dot:             # (the diagonal decoder scores a chain by the plain dot product)
                    return q @ cand.t()
                return F.normalize(q, dim=1) @ F.normalize(cand, dim=1).t()

            def torch_rank():
                s = cosines()
                return 1 + (s > s.gather(1, target_rows[:, None])).sum(dim=1)

            def in_mode(training, fn):
                def run():
                    model.train(training)
                    return fn()
                return run
            row = {'formula': repr(f), 'entities_of_target_mode': int(len(ids_all)), 'rows_ranked': int(n)}
            with torch.no_grad():
                cases = [('fused_answer', in_mode(True, lambda: model.answer(f, qs, k=a.k))),
                         ('fused_rank_targets', in_mode(True, lambda: model.rank_targets(f, qs))),
                         ('torch_topk', lambda: torch.topk(cosines(), a.k, dim=1)),
                         ('torch_rank', torch_rank),
                         ('forward_all_negatives', lambda: model.forward(f, qs, targets, neg_nodes=negs, neg_lengths=lens))]
                if 'inter' not in qt:
                    cases[2:2] = [('fused_answer_cached', in_mode(False, lambda: model.answer(f, qs, k=a.k))),
                                  ('fused_rank_targets_cached', in_mode(False, lambda: model.rank_targets(f, qs)))]
                for name, fn in cases:
                    med, lo, hi = timed(fn, a.warmup, a.blocks, a.iters)
                    row[name + '_ms'] = {'median': med, 'min': lo, 'max': hi}
                model.eval()
                ids, _ = model.answer(f, qs, k=a.k)
                base = torch.topk(cosines(), a.k, dim=1)[1]
                row['top1_agrees_with_torch'] = float((model._mode_rows(f.target_mode, ids.device)[0][base[:, 0]] == ids[:, 0]).float().mean())
            row['torch_over_fused_answer'] = row['torch_topk_ms']['median'] / row['fused_answer_ms']['median']
            row['forward_over_fused_answer'] = row['forward_all_negatives_ms']['median'] / row['fused_answer_ms']['median']
            per_type[qt] = row
        out['shapes'][kg] = per_type
        del model
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kgs', nargs='+', default=['aifb', 'mutag', 'am'])
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--model', default='rgcn', choices=['rgcn', 'gqe'])
    ap.add_argument('--decoder', default='bilinear', choices=['bilinear', 'transe', 'bilinear-diag'],
                    help='gqe: the metapath decoder')
    ap.add_argument('--inter-decoder', default='mean', help='gqe: mean | min | mean-simple | min-simple')
    ap.add_argument('--query-types', nargs='+', default=['1-chain', '2-chain', '3-chain', '2-inter', '3-inter', '3-inter_chain',
                                                         '3-chain_inter'], help='gqe: the query types timed')
    a = ap.parse_args()
    if a.model == 'gqe':
        return main_gqe(a)
    from mpqe_amd import ops, synthetic
    torch.cuda.set_device(0)
    out = {'tool': 'answer_bench', 'batch': a.batch, 'dim': a.dim, 'k': a.k, 'query_type': '2-chain',
           'timing': 'device events, median of %d blocks of %d calls after %d warm-up calls' % (a.blocks, a.iters, a.warmup),
           'shapes': {}}
    for kg in a.kgs:
        schema, model = build(kg, a.dim)
        model = model.to('cuda:0').eval()
        rng = np.random.RandomState(1)
        f = synthetic.sample_formula(schema, '2-chain', rng)
        qs = synthetic.sample_queries(schema, f, a.batch, rng, n_neg=1, n_hard=1)
        n = len(schema.ids[f.target_mode])
        with torch.no_grad():
            q = model._query_embeddings(f, qs, None, None, None).clone()
            table = model.enc.table(f.target_mode).detach()[:n]
            targets = torch.from_numpy(np.array([q_.target_node for q_ in qs], dtype=np.int64)).to('cuda:0')
            target_rows = model.enc.node_maps[targets]

            def baseline_topk():
                t = F.normalize(table, dim=1)
                s = F.normalize(q, dim=1) @ t.t()
                return torch.topk(s, a.k, dim=1)

            def baseline_rank():
                t = F.normalize(table, dim=1)
                s = F.normalize(q, dim=1) @ t.t()
                return 1 + (s > s.gather(1, target_rows[:, None])).sum(dim=1)

            row = {'entities_of_target_mode': n}
            for name, fn in (('answer', lambda: model.answer(f, qs, k=a.k)),
                             ('rank_targets', lambda: model.rank_targets(f, qs)),
                             ('kernel_topk', lambda: ops.rank_entities(q, table, None, None, a.k)),
                             ('kernel_rank', lambda: ops.rank_entities(q, table, target_rows, None, 0)),
                             ('baseline_gemm_topk', baseline_topk),
                             ('baseline_gemm_rank', baseline_rank)):
                med, lo, hi = timed(fn, a.warmup, a.blocks, a.iters)
                row[name + '_ms'] = {'median': med, 'min': lo, 'max': hi}
            flops = 2.0 * a.batch * n * a.dim
            row['kernel_topk_share_of_fp32_mfma_roof'] = flops / (row['kernel_topk_ms']['median'] * 1e-3) / (PEAK_FP32_MATRIX_TFLOPS * 1e12)
            row['baseline_over_kernel_topk'] = row['baseline_gemm_topk_ms']['median'] / row['kernel_topk_ms']['median']
            row['baseline_over_kernel_rank'] = row['baseline_gemm_rank_ms']['median'] / row['kernel_rank_ms']['median']
            ids, _ = model.answer(f, qs, k=a.k)
            base = baseline_topk()[1]
            row['top1_agrees_with_baseline'] = float((model._mode_rows(f.target_mode, q.device)[0][base[:, 0]] == ids[:, 0]).float().mean())
        out['shapes'][kg] = row
        del model, table, q
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
