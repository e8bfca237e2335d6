"""gd_spmm_csr_onepass_wide_f32: the 64-float aggregation with up to 16 consecutive light rows per item, summed by the fp32
matrix instruction, hub rows on the vector path inside the same launch.  Against the fp64 dense product, against the two-row
form of the vector kernel (GD_SPMM_D64_FORM=pairs), run to run, and under a captured graph - with and without edge weights,
bias, self term (coefficient 0 / 1 / 0.5 from a separate matrix), at row pitches 64 and 80, on the full plan and a row subset."""
import pytest
import torch

from helpers import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5          # the bound tests/test_kernels_gpu.py holds every kernel to against the fp64 product
FORMS = 1e-6        # ... and the one it holds two forms of the aggregation to against each other
N, D = 4100, 64     # (4100 rows: not a multiple of 16, the last item is a partial one)
HUBS = {199: 65, 217: 129, 299: 1000, 340: 70, 399: 66, 499: 65}


@pytest.fixture(scope='module')
def case():
    from gnndelete_amd.graph import SplitPlan, build_csr
    g = torch.Generator().manual_seed(11)
    deg = torch.randint(0, 15, (N,), generator=g)                  # about 30 k random edges
    deg[0], deg[N - 1] = 5, 3
    deg[50:70] = 0                                                 # a run of rows without in-edges
    deg[100:130] = 1                                               # ... and of rows with one
    deg[200:217] = 2                                               # 17 light rows between two hubs: an item of 16 + 1
    deg[300:340] = 1                                               # 40 between two hubs: 16 + 16 + 8
    deg[400:404], deg[404] = 16, 1                                 # an item that fills exactly 64 edges, and the row after it
    deg[500], deg[501] = 64, 5                                     # a single row of 64 edges
    for r, k in HUBS.items():
        deg[r] = k
    dst = torch.repeat_interleave(torch.arange(N), deg)
    src = torch.randint(0, N, (int(deg.sum()),), generator=g)
    gr = build_csr(torch.stack([src, dst]).cuda(), N, 'sum')
    rowptr, col = gr.rowptr.cpu().long(), gr.col.cpu().long()
    assert torch.equal(rowptr[1:] - rowptr[:-1], deg)
    val = torch.rand(col.shape[0], generator=g) + 0.25
    rt = torch.repeat_interleave(torch.arange(N), deg)
    a_w = torch.zeros(N, N, dtype=torch.float64).index_put_((rt, col), val.double(), accumulate=True)
    a_1 = torch.zeros(N, N, dtype=torch.float64).index_put_((rt, col), torch.ones(col.shape[0], dtype=torch.float64), accumulate=True)
    x, xs, b = torch.randn(N, D, generator=g), torch.randn(N, D, generator=g), torch.randn(D, generator=g)
    rows = torch.cat([torch.randperm(N, generator=g)[:int(0.6 * N)], torch.tensor([0, N - 1, 500] + list(HUBS))]).unique()
    sub = SplitPlan(gr.rowptr, rows=rows.cuda())
    items = gr.plan.onepass_wide(D)[0]
    nr = -items[(items[:, 0] >= 0) & (items[:, 3] <= -16)][:, 3] - 15
    assert int(nr.max()) == 16 and int((items[:, 3] == -2).sum()) == 4 * len(HUBS)
    return dict(gr=gr, val=val.cuda(), ax={True: a_w @ x.double(), False: a_1 @ x.double()}, x=x, xs=xs, b=b,
                plans={'full': (gr.plan, torch.arange(N)), 'subset': (sub, rows)}, hub=torch.tensor(sorted(HUBS)))


def _padded(t, pitch):
    buf = torch.full((t.shape[0], pitch), 3.0, device='cuda')
    buf[:, :t.shape[1]] = t.cuda()
    return buf


@pytest.mark.parametrize('self_coef', [0.0, 1.0, 0.5])
@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('weighted', [True, False])
def test_wide_spmm_matches_dense_product_and_pairs_form(case, weighted, with_bias, self_coef, monkeypatch):
    from gnndelete_amd import ops
    gr = case['gr']
    val = case['val'] if weighted else None
    bias = case['b'].cuda() if with_bias else None
    want = case['ax'][weighted] + self_coef * case['xs'].double() + (case['b'].double() if with_bias else 0.0)
    wide_calls = []
    wide_col = ops._wide_col
    monkeypatch.setattr(ops, '_wide_col', lambda *a: wide_calls.append(1) or wide_col(*a))
    for pitch in (64, 80):
        xb, xsb = _padded(case['x'], pitch), _padded(case['xs'], pitch)
        xv, xsv = xb[:, :D], xsb[:, :D]
        for name, (plan, rows) in case['plans'].items():
            def run():
                yb = torch.full((N, pitch), 7.0, device='cuda')
                ops._spmm_raw(gr.rowptr, gr.col, val, xv, bias, self_coef, N, plan, out=yb[:, :D], x_self=xsv)
                return yb
            n_wide = len(wide_calls)
            yb = run()
            assert len(wide_calls) == n_wide + 1                                 # the wide entry took the call
            y = yb[:, :D].cpu()
            err = rel_l2(y[rows], want[rows])
            print(f'pitch {pitch} {name}: rel-L2 to the fp64 product {err:.2e}')
            assert err < TOL
            rest = torch.ones(N, dtype=torch.bool)
            rest[rows] = False
            assert bool((y[rest] == 7.0).all()) and bool((yb[:, D:] == 7.0).all())      # rows outside the plan, pad columns
            assert bool((xb[:, D:] == 3.0).all())
            assert torch.equal(yb, run())                                         # run to run
            monkeypatch.setenv('GD_SPMM_D64_FORM', 'pairs')
            yp = run()
            monkeypatch.delenv('GD_SPMM_D64_FORM')
            assert len(wide_calls) == n_wide + 2                                 # ... and not that one
            diff = rel_l2(y[rows], yp[:, :D].cpu()[rows])
            print(f'pitch {pitch} {name}: rel-L2 to the pairs form {diff:.2e}')
            assert diff < FORMS
            assert torch.equal(yb[case['hub'].cuda()], yp[case['hub'].cuda()])    # hub rows: the same sum, bit for bit
            yg = torch.full((N, pitch), 7.0, device='cuda')
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ops._spmm_raw(gr.rowptr, gr.col, val, xv, bias, self_coef, N, plan, out=yg[:, :D], x_self=xsv)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(yg, yb)


def test_wide_spmm_is_not_selected_with_one_row_items(case, monkeypatch):
    """GD_SPMM_MULTIROW=0 keeps the one-row items of the vector kernel."""
    from gnndelete_amd import ops
    from gnndelete_amd.graph import SplitPlan
    gr = case['gr']
    calls = []
    wide_col = ops._wide_col
    monkeypatch.setattr(ops, '_wide_col', lambda *a: calls.append(1) or wide_col(*a))
    monkeypatch.setenv('GD_SPMM_MULTIROW', '0')
    plan1 = SplitPlan(gr.rowptr)
    y = ops._spmm_raw(gr.rowptr, gr.col, None, case['x'].cuda(), None, 0.0, N, plan1)
    assert not calls and int((plan1.onepass(D)[0][:, 3] <= -16).sum()) == 0
    assert rel_l2(y.cpu(), case['ax'][False]) < TOL


def test_wide_entry_checks_its_arguments(case):
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import ptr
    gr = case['gr']
    items, n_items, bounds, tags = gr.plan.onepass_wide(D)
    colt = gr.col | (tags << 24)
    x = torch.zeros(N, 128, device='cuda')
    y = torch.zeros(N, 128, device='cuda')

    def call(d, x_rows, n_it=n_items, yy=y):
        return _lib.lib().gd_spmm_csr_onepass_wide_f32(ptr(items), n_it, ptr(colt), None, ptr(x), 128, ptr(yy), 128, None, 0.0, None, d,
                                                       int(colt.shape[0]), x_rows, ptr(bounds), None)
    assert call(128, N) == 2                                                     # GD_E_DIM: d must be 64
    assert call(64, 0) == 2 and call(64, 1 << 24) == 2                           # 24-bit addressing conditions
    assert call(64, N, n_it=n_items - 1) == 2 and call(64, N, yy=x) == 2
    assert call(64, N, n_it=0) == 0
