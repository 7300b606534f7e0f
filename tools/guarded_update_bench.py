"""What the guard costs the dense update: mpqe_adam_step_guarded / mpqe_sgd_step_guarded against mpqe_adam_step /
mpqe_sgd_step (the same kernel without the word) in one process, alternating, on the flat size of the AIFB D = 128 model and
on 64 Mi elements. Event timings of groups of launches, a warm-up first, medians over --reps groups each and the spread of
both. The guard is one 4-byte load per workgroup of an HBM-bound launch (16 B read + 12 B written per element).

    python tools/guarded_update_bench.py [--reps 9] [--out profiles/guarded_update.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def aifb_flat_size(D=128):
    from mpqe_amd import synthetic
    from mpqe_amd.data_utils import make_feature_modules
    from mpqe_amd.encoders import DirectEncoder
    from mpqe_amd.model import RGCNEncoderDecoder
    schema = synthetic.make_schema(*synthetic.KG_SHAPES['aifb'], seed=0)
    graph = synthetic.SchemaGraph(schema, D)
    fm, node_maps = make_feature_modules(schema.ids, D, schema.num_entities)
    model = RGCNEncoderDecoder(graph, DirectEncoder(None, fm, node_maps), readout='mp', num_layers=3, shared_layers=False,
                               adaptive=True, weight_decay=0)
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def measure(lib, kind, n, reps, group):
    dev = torch.device('cuda:0')
    p, g, m = (torch.randn(n, device=dev) * 0.1 for _ in range(3))
    v = torch.rand(n, device=dev) * 0.01
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    applied = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    t = [0]

    def call(guarded):
        t[0] += 1
        if kind == 'adam':
            args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 0.0, t[0])
        else:
            args = (p.data_ptr(), g.data_ptr(), n, 1e-3, 0.0)
        if guarded:
            st = getattr(lib, 'mpqe_%s_step_guarded' % kind)(*(args + (word.data_ptr(), applied.data_ptr(), stream)))
        else:
            st = getattr(lib, 'mpqe_%s_step' % kind)(*(args + (stream,)))
        assert st == 0, st

    def timed(guarded):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(group):
            call(guarded)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / group          # us per launch

    for _ in range(3):
        timed(False)
        timed(True)
    us = {False: [], True: []}
    for _ in range(reps):                               # alternating: drift of the clocks lands on both alike
        for guarded in (False, True):
            us[guarded].append(timed(guarded))
    torch.cuda.synchronize()
    assert int(applied.item()) == (3 + reps) * group

    def summary(x):
        q = np.percentile(x, [25, 75])
        return {'median_us': statistics.median(x), 'min_us': min(x), 'max_us': max(x), 'iqr_us': float(q[1] - q[0])}
    u, gd = summary(us[False]), summary(us[True])
    bytes_moved = n * (28 if kind == 'adam' else 12)
    return {'kind': kind, 'n': n, 'launches_per_timing': group, 'timings_each': reps, 'unguarded': u, 'guarded': gd,
            'unguarded_GBps': bytes_moved / u['median_us'] / 1e3, 'guarded_GBps': bytes_moved / gd['median_us'] / 1e3,
            'guarded_median_within_unguarded_spread': bool(u['min_us'] <= gd['median_us'] <= u['max_us'])}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from mpqe_amd import ops
    torch.cuda.set_device(0)
    lib = ops.lib()
    n_aifb = aifb_flat_size()
    out = {'what': 'dense update, guarded entry point against the unguarded one (the same kernel, no word), alternating in one '
                   'process; event timings of groups of launches, us per launch',
           'device': torch.cuda.get_device_name(0), 'cases': []}
    for kind in ('adam', 'sgd'):
        for n, group in ((n_aifb, 50), (64 << 20, 5)):
            out['cases'].append(measure(lib, kind, n, a.reps, group))
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
