"""The two 64-float aggregations of the bench step (spmm2: forward with bias, spmm2_t: transposed), wide form
(gd_spmm_csr_onepass_wide_f32) against GD_SPMM_D64_FORM=pairs, alternating in one process on the step's own graph: HIP events,
20 launches a round, three rounds each, for a few rows per item / visit costs of the plan / grid caps (0 = the default).
AB_SET=2 runs the second set of variants, AB_ONLY=1 the default alone (the run the counter passes profile).
Results: profiles/spmm_wide_ab.txt."""
import os, sys, torch
sys.path.insert(0, '.')
import bench
from gnndelete_amd import ops, graph as G
sys.argv = ['bench.py']
args = bench.parse()
dev = torch.device('cuda', 0)
data, model, neg, ni1, ni2 = bench.build_request(args, dev)
eng = bench.make_engine(args, data, model, neg, ni1, ni2, dev)
g, n = eng.graph, eng.n


def timed(fn, reps=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


torch.manual_seed(0)
x = torch.randn(n, 64, device=dev)
b = torch.randn(64, device=dev)
variants = [(16, 24, 0), (16, 24, 1024), (16, 24, 4096), (16, 24, 8192), (8, 24, 0), (8, 24, 4096), (16, 8, 0), (16, 48, 0), (16, 64, 0)]
if os.environ.get('AB_SET') == '2':
    variants = [(16, 24, 0), (16, 64, 0), (16, 96, 0), (16, 24, 8192), (16, 64, 8192), (8, 24, 0), (12, 24, 0)]
only = os.environ.get('AB_ONLY')
if only:
    variants = variants[:1]
for tr in (False, True):
    rp, col, val, plan = (g.rowptr_t, g.col_t, g.val_t, g.plan_t) if tr else (g.rowptr, g.col, g.val, g.plan)
    bias = None if tr else b
    name = 'spmm2_t' if tr else 'spmm2'
    y = torch.empty_like(x)
    os.environ['GD_SPMM_D64_FORM'] = 'pairs'
    ops._spmm_raw(rp, col, val, x, bias, 0.0, n, plan, out=y)
    torch.cuda.synchronize()
    ref = y.clone()
    print(f'{name}: pairs items {plan.onepass(64)[1]}', flush=True)
    for rows, cost, cap in variants:
        G.WIDE_ROWS, G.WIDE_VISIT_COST = rows, cost
        if cap: os.environ['GD_SPMM_GRID_CAP'] = str(cap)
        else: os.environ.pop('GD_SPMM_GRID_CAP', None)
        os.environ['GD_SPMM_D64_FORM'] = ''
        y.zero_()
        ops._spmm_raw(rp, col, val, x, bias, 0.0, n, plan, out=y)
        torch.cuda.synchronize()
        rel = float((y - ref).norm() / ref.norm())
        mx = float((y - ref).abs().max())
        tw, tp = [], []
        for _ in range(3):
            os.environ['GD_SPMM_D64_FORM'] = ''
            tw.append(timed(lambda: ops._spmm_raw(rp, col, val, x, bias, 0.0, n, plan, out=y)))
            os.environ['GD_SPMM_D64_FORM'] = 'pairs'
            cap_env = os.environ.pop('GD_SPMM_GRID_CAP', None)
            tp.append(timed(lambda: ops._spmm_raw(rp, col, val, x, bias, 0.0, n, plan, out=y)))
            if cap_env: os.environ['GD_SPMM_GRID_CAP'] = cap_env
        print(f'{name} rows/item {rows:2d} visit cost {cost:2d} cap {cap or "default":>7} items {plan.onepass_wide(64)[1]:6d}: wide '
              f'{min(tw):6.1f} us ({" ".join(f"{t:.1f}" for t in tw)})  pairs {min(tp):6.1f} us ({" ".join(f"{t:.1f}" for t in tp)})  '
              f'rel diff {rel:.1e} max abs {mx:.1e}', flush=True)
os.environ['GD_SPMM_D64_FORM'] = ''
