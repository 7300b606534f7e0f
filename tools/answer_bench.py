"""Time of answering a batch of queries over ALL entities of the target mode -- RGCNEncoderDecoder.answer (k = 10) and
rank_targets, the fused score / count / top-k kernel of csrc/rank.hip -- on KG shapes of synthetic.KG_SHAPES at B = 512,
D = 128, beside what a user could write before it: F.normalize(table) -> q_normalised @ t.T -> torch.topk (the library
GEMM, the [B, N] score matrix materialised), fed the same query embeddings.

Device-event timing: warm-up, then `--blocks` blocks of `--iters` calls, one event pair per block, the median block
reported per call. `kernel_*` rows time ops.rank_entities alone (no encoder, no id translation), which is what the
baseline's three ops compare with; `answer` / `rank_targets` are the whole calls, encoder included.

    python tools/answer_bench.py [--kgs aifb mutag am] [--batch 512] [--dim 128]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kgs', nargs='+', default=['aifb', 'mutag', 'am'])
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--iters', type=int, default=10)
    a = ap.parse_args()
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
