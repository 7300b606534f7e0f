"""Time of one forward + backward of the neighbourhood-aggregating Encoder (mpqe_amd/encoders.py, the reference's
`--depth 1..3`) with and without `index=`: the device path (draws on the KG index, ONE encode launch: csrc/sage.hip) beside
the host path it leaves in place (one random.sample per node and relation in Python, then a features lookup, a scatter-mean
and an accumulating dense layer per relation). Same module, same parameters, same batch; the two paths alternate in one
process. Device events around each call (a call ends in the backward's last launch), medians of --blocks timed calls after
--warmup, min and max beside them. The draws differ (the library's stream against Python's), the work per call does not.

  aifb   the AIFB-shaped graph (2 601 entities, synthetic.make_adjacency): both paths; depth 1 at B = 512, depth 2 at B = 64
  am     an AM-shaped random graph (372 584 entities) through KGIndex.from_edges: no Python adjacency, device path only

--profile: only the device path at depth 1, over random edges (KGIndex.from_edges, --am-degree) for every KG, --blocks calls,
for a `rocprofv3 --kernel-trace --stats` run of its own; the JSON line then
carries the algorithmic bytes of one forward (4 dim_in (sum of counts + B) gathered, W, the output) to set against the
kernels' times.

    python tools/sage_bench.py [--kgs aifb am] [--out profiles/sage_bench.json]
    rocprofv3 --kernel-trace --stats -- python tools/sage_bench.py --kgs aifb --profile
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def build(kg, depth, D, args, device, host):
    """-> (device encoder, host encoder or None, graph): one set of parameters"""
    import kg_answers_bench as kab
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.kg import KGIndex
    from mpqe_amd.utils import get_encoder
    schema = synthetic.make_schema(*synthetic.KG_SHAPES[kg], seed=args.seed)
    torch.manual_seed(args.seed)
    fm, node_maps = make_feature_modules(schema.ids, D, schema.num_entities)
    graph = synthetic.SchemaGraph(schema, D)
    if host:
        graph.adj_lists = synthetic.make_adjacency(schema, degree=args.degree, seed=args.seed)
        index = KGIndex.from_graph(graph, node_maps, device)
    else:
        index = KGIndex.from_edges(schema, kab.random_edges(schema, args.am_degree, args.seed), node_maps, device)
    maps_dev = node_maps.to(device)

    def features(nodes, mode):
        # (the null neighbour of a node without edges reads the padding row, which the reference's closure cannot)
        ids = torch.as_tensor(nodes, dtype=torch.long, device=device)
        table = fm[mode]
        return table(torch.where(ids < 0, torch.full_like(ids, table.weight.shape[0] - 1), maps_dev[ids.clamp(min=0)]))
    graph.features = features
    dims = {m: D for m in schema.modes}
    dev_enc = get_encoder(depth, graph, dims, fm, True, node_maps=node_maps, index=index).to(device)
    host_enc = None
    if host:
        host_enc = get_encoder(depth, graph, dims, fm, True, node_maps=node_maps).to(device)
        host_enc.load_state_dict(dev_enc.state_dict(), strict=True)
    return dev_enc, host_enc, graph


def timed(enc, nodes, mode, gout, args):
    enc.zero_grad()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = enc(nodes, mode, keep_prob=args.keep_prob, max_keep=args.max_keep)
    out.backward(gout)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], calls=len(ms))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--kgs', nargs='+', default=['aifb', 'am'])
    ap.add_argument('--embed-dim', type=int, default=128)
    ap.add_argument('--keep-prob', type=float, default=0.5)
    ap.add_argument('--max-keep', type=int, default=10)
    ap.add_argument('--degree', type=int, default=2)
    ap.add_argument('--am-degree', type=int, default=4)
    ap.add_argument('--blocks', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    device = torch.device('cuda:0')
    D = args.embed_dim
    rows = []
    shapes = [(kg, depth, B) for kg in args.kgs for depth, B in ((1, 512), (2, 64))]
    if args.profile:
        shapes = [(kg, 1, 512) for kg in args.kgs]
    for kg, depth, B in shapes:
        host = kg == 'aifb' and not args.profile
        dev_enc, host_enc, graph = build(kg, depth, D, args, device, host)
        mode = max(graph.relations, key=lambda m: len(graph.relations[m]))
        rng = np.random.RandomState(args.seed + 1)
        nodes = [int(x) for x in rng.choice(graph.schema.ids[mode], size=B, replace=True)]
        ids_dev = torch.tensor(nodes, dtype=torch.int64, device=device)
        gout = torch.randn((D, B), generator=torch.Generator().manual_seed(1)).to(device)
        random.seed(args.seed)
        times = {'device': [], 'host': []}
        blocks = args.blocks if depth == 1 or not host else max(args.blocks // 4, 3)
        for it in range(args.warmup + blocks):
            for name, enc, batch in (('device', dev_enc, ids_dev), ('host', host_enc, nodes)):
                if enc is None:
                    continue
                ms = timed(enc, batch, mode, gout, args)
                if it >= args.warmup:
                    times[name].append(ms)
        counts = dev_enc.last_sample['counts']
        R = len(graph.relations[mode])
        row = dict(kg=kg, depth=depth, batch=B, dim=D, mode=mode, relations=R, keep_prob=args.keep_prob, max_keep=args.max_keep,
                   sampled_rows=int(counts.sum().item()), device=stats(times['device']))
        # one forward of the outer layer: rows gathered, the compress matrix, the output
        row['forward_bytes'] = 4 * D * (row['sampled_rows'] + int((counts == 0).sum().item()) + B) + 4 * D * (R + 1) * D + 4 * B * D
        if times['host']:
            row['host'] = stats(times['host'])
            row['host_over_device'] = row['host']['median_ms'] / row['device']['median_ms']
        assert int(dev_enc._err.item()) == 0
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            for row in rows:
                f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
