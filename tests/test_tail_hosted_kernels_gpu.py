"""gd_spmm_csr_onepass_wide_hosted_f32: the wide 64-float aggregation whose launch carries the step tail's jobs (W_D1's column job;
W_D2's reduction + Adam and the loss finalize) as extra blocks in front of the sweep.

Every assertion is on bits: y against gd_spmm_csr_onepass_wide_f32 on the same operands, every tail output against
gd_step_tail_fold1_f32 on clones of the same inputs, `arrive` back at 0, the same bits twice, sentinels around every output intact.
Graph: 4,099 nodes (the last item is short), mean in-degree about 6, one row of 300 in-edges (GROUP items), a run of 40
self-loop-only rows.  Partial counts: the boundaries of the `b + 56 <` / `b + 48 <` loops and of the 8- / 16-slot slices.  Grids: a
4-item launch (fewer sweep blocks than job blocks) and GD_SPMM_GRID_CAP=8 (every sweep wave makes many visits)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
N, D, O, H = 4099, 64, 64, 128
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
CAP = 8                                        # rows of the loss history ring
N1 = (1, 7, 8, 57, 64, 65, 256)                # partial matrices of job 1 ...
N2 = (1, 15, 16, 17, 49, 64, 65, 256)          # ... and of job 2
PAD = 32                                       # sentinel elements on either side of every output
OUT1 = ('g1', 'wd', 'm1', 'v1', 'wf', 'bf')
OUT2 = ('g2', 'wd2', 'm2', 'v2', 'hist', 'pos', 'iter', 'arrive')


def _lib():
    from gnndelete_amd import _lib
    return _lib.lib()


def _p(t):
    from gnndelete_amd._lib import ptr
    return ptr(t)


def _build(n, hub=None, loops=None, seed=5):
    from gnndelete_amd.graph import build_csr
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 11, (n,), generator=g)                   # + the self loop build_csr adds: about 6 in-edges per row
    if hub is not None:
        deg[hub] = 299
    if loops is not None:
        deg[loops[0]:loops[1]] = 0
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = (dst + 1 + torch.randint(0, n - 1, (int(deg.sum()),), generator=g)) % n          # (never the row itself)
    if hub is not None:
        src[dst == hub] = (hub + 1 + torch.arange(299)) % n                                  # (distinct sources)
    gr = build_csr(torch.stack([src, dst]).cuda(), n, 'gcn')
    x = torch.randn(n, D, generator=g).cuda()
    b = torch.randn(D, generator=g).cuda()
    return gr, x, b


@functools.lru_cache(maxsize=None)
def _graph():
    gr, x, b = _build(N, hub=1234, loops=(2000, 2040))
    indeg = (gr.rowptr[1:] - gr.rowptr[:-1]).cpu()
    items = gr.plan.onepass_wide(D)[0].cpu()
    assert int(indeg[1234]) >= 300 and bool((indeg[2000:2040] == 1).all()) and 5.0 < float(indeg.float().mean()) < 7.5
    assert int((items[:, 3] == -2).sum()) >= 4 and N % 16 == 3            # GROUP items; the last item holds three rows
    return gr, x, b


@functools.lru_cache(maxsize=None)
def _tiny():
    gr, x, b = _build(8, seed=9)                                           # eight rows, fewer than 64 in-edges together: one item
    assert gr.plan.onepass_wide(D)[1] == 4                                 # ... and its padding: 8 sweep blocks behind 192 job blocks
    return gr, x, b


def _state(n1, n2, it, pos, seed=0):
    gen = torch.Generator(device='cuda').manual_seed(1000 * n1 + n2 + seed)
    r = lambda *sh: torch.randn(*sh, device='cuda', generator=gen)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device='cuda')
    return dict(parts1=r(n1, H, H), cs=r(n1, H), w1=0.1 * r(H, H), b1=0.1 * r(H), parts2=r(n2, O, O), lp1=r(2 * 300).abs(), lp2=r(2 * 7).abs(),
                g1=r(H, H), wd=(torch.eye(H, device='cuda') + 0.05 * r(H, H)).contiguous(), m1=1e-3 * r(H, H), v1=1e-6 * r(H, H).abs(),
                wf=r(H, H), bf=r(H), g2=r(O, O), wd2=(torch.eye(O, device='cuda') + 0.05 * r(O, O)).contiguous(), m2=1e-3 * r(O, O),
                v2=1e-6 * r(O, O).abs(), hist=r(CAP, 4), pos=i32(pos), iter=i32(it), arrive=i32(0, 0))


def _reference(st, acc2):
    """Everything gd_step_tail_fold1_f32 writes, on clones."""
    o = {k: v.clone() for k, v in st.items()}
    rc = _lib().gd_step_tail_fold1_f32(_p(o['parts1']), _p(o['cs']), o['parts1'].shape[0], H, 0, _p(o['w1']), _p(o['b1']), _p(o['g1']), _p(o['wd']),
                                       _p(o['m1']), _p(o['v1']), _p(o['wf']), _p(o['bf']), _p(o['parts2']), o['parts2'].shape[0], O, acc2, _p(o['g2']),
                                       _p(o['wd2']), _p(o['m2']), _p(o['v2']), LR, B1, B2, EPS, _p(o['lp1']), 300, _p(o['lp2']), 7, _p(o['hist']), CAP,
                                       _p(o['pos']), _p(o['iter']), _p(o['arrive']), None)
    assert rc == 0
    torch.cuda.synchronize()
    return o


def _guarded(t):
    """-> (a copy of t inside a buffer with PAD sentinel elements on either side, the buffer)."""
    sent = 7 if t.dtype == torch.int32 else 7.0
    buf = torch.full((t.numel() + 2 * PAD,), sent, dtype=t.dtype, device='cuda')
    view = buf[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def _host_args(o, job1, job2, acc2):
    return (_p(o['parts1']), _p(o['cs']), o['parts1'].shape[0] if job1 else 0, H, _p(o['w1']), _p(o['w1t']), _p(o['b1']), _p(o['g1']), _p(o['wd']),
            _p(o['m1']), _p(o['v1']), _p(o['wf']), _p(o['bf']), _p(o['parts2']), o['parts2'].shape[0] if job2 else 0, O, acc2, _p(o['g2']),
            _p(o['wd2']), _p(o['m2']), _p(o['v2']), LR, B1, B2, EPS, _p(o['lp1']), 300, _p(o['lp2']), 7, _p(o['hist']), CAP, _p(o['pos']),
            _p(o['iter']), _p(o['arrive']))


def _hosted(case, st, job1, job2, acc2):
    """One hosted launch on guarded clones -> (outputs, their buffers, y inside its sentinel rows and pad columns)."""
    from gnndelete_amd import ops
    gr, x, b = case
    o, bufs = {}, {}
    for k, v in st.items():
        o[k], bufs[k] = _guarded(v) if k in OUT1 + OUT2 else (v.clone(), None)
    o['w1t'] = st['w1'].t().contiguous()
    n = x.shape[0]
    yb = torch.full((n + 2, 80), 7.0, device='cuda')
    ops._spmm_raw(gr.rowptr, gr.col, gr.val, x, b, 0.0, n, gr.plan, out=yb[1:n + 1, :D], host=_host_args(o, job1, job2, acc2))
    torch.cuda.synchronize()
    return o, bufs, yb


def _plain(case):
    from gnndelete_amd import ops
    gr, x, b = case
    n = x.shape[0]
    yb = torch.full((n + 2, 80), 7.0, device='cuda')
    ops._spmm_raw(gr.rowptr, gr.col, gr.val, x, b, 0.0, n, gr.plan, out=yb[1:n + 1, :D])
    torch.cuda.synchronize()
    return yb


def _check(case, n1, n2, it=5, pos=2, job1=True, job2=True, acc2=0):
    st = _state(n1, n2, it, pos)
    ref = _reference(st, acc2)
    y_ref = _plain(case)
    assert bool((y_ref[0] == 7.0).all()) and bool((y_ref[-1] == 7.0).all()) and bool((y_ref[:, D:] == 7.0).all())
    first = None
    for _ in range(2):                                                      # the same bits twice
        o, bufs, yb = _hosted(case, st, job1, job2, acc2)
        assert torch.equal(yb, y_ref)                                       # y, its pad columns and the rows around it
        for k in OUT1 + OUT2:
            want = ref[k] if (k in OUT1 and job1) or (k in OUT2 and job2) else st[k]           # a job left out writes nothing
            assert torch.equal(o[k], want), k
            sent = 7 if o[k].dtype == torch.int32 else 7.0
            assert bool((bufs[k][:PAD] == sent).all()) and bool((bufs[k][-PAD:] == sent).all()), k
        assert int(o['arrive'][0]) == 0 and int(o['arrive'][1]) == 0
        if job2:
            assert int(o['iter']) == it + 1 and int(o['pos']) == (pos + 1) % CAP
        if first is not None:
            for k in OUT1 + OUT2:
                assert torch.equal(o[k], first[k]), k
        first = o


@pytest.mark.parametrize('n1,n2', list(zip(N1 + (256,), N2)))
def test_partial_counts(n1, n2):
    _check(_graph(), n1, n2)


@pytest.mark.parametrize('acc2', [0, 1])
@pytest.mark.parametrize('it', [0, 5])
def test_accumulate_flag_and_iteration_counter(acc2, it):
    _check(_graph(), 65, 17, it=it, acc2=acc2)


def test_history_position_wraps():
    _check(_graph(), 8, 16, pos=CAP - 1)


@pytest.mark.parametrize('job1,job2', [(True, False), (False, True)])
def test_one_job_alone(job1, job2):
    _check(_graph(), 57, 49, job1=job1, job2=job2, acc2=1)


def test_fewer_sweep_blocks_than_job_blocks():
    _check(_tiny(), 64, 64)


def test_under_a_grid_cap_of_eight_blocks(monkeypatch):
    monkeypatch.setenv('GD_SPMM_GRID_CAP', '8')
    _check(_graph(), 65, 65)


def test_refusals():
    gr, x, b = _graph()
    L = _lib()
    items, n_items, bounds, tags = gr.plan.onepass_wide(D)
    colt = (gr.col | (tags << 24)).contiguous()
    y = torch.zeros(N, D, device='cuda')
    st = _state(8, 16, 0, 0)
    st['w1t'] = st['w1'].t().contiguous()
    keep = {k: v.clone() for k, v in st.items()}

    def call(n_it=n_items, d=D, **chg):
        o = dict(st)
        o.update({k: v for k, v in chg.items() if k in o})
        host = list(_host_args(o, chg.get('job1', True), chg.get('job2', True), 0))
        for i, v in chg.get('at', {}).items():
            host[i] = v
        return L.gd_spmm_csr_onepass_wide_hosted_f32(_p(items), n_it, _p(colt), _p(gr.val), _p(x), D, _p(y), D, _p(b), 0.0, None, d, int(colt.shape[0]),
                                                     N, _p(bounds), *host, None)
    assert call(job1=False, job2=False) == 2                                # GD_E_DIM: no job at all
    assert call(at={2: -1}) == 2 and call(at={14: -1}) == 2                  # negative partial counts
    assert call(at={3: 64}) == 2                                            # d1 must be 128
    assert call(at={15: 6}) == 2 and call(at={15: 0}) == 2                   # d2 % 4, d2 > 0
    assert call(n_it=0) == 2                                                # nothing to ride on
    assert call(d=128) == 2 and call(n_it=n_items - 1) == 2                 # the unhosted entry's own conditions
    for i in (0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12):                           # null pointers of job 1
        assert call(at={i: None}) == 1, i
    for i in (13, 17, 18, 19, 20, 29, 31, 33):                               # ... of job 2 and of the bookkeeping
        assert call(at={i: None}) == 1, i
    assert call(at={32: None}) == 1                                         # the iteration counter, whichever job
    assert call(job1=False, at={0: None, 4: None, 5: None}) == 0             # a job left out: its pointers are not read
    torch.cuda.synchronize()
    assert call(at={30: 0}) == 1                                            # capacity
    for k in ('parts1', 'cs', 'w1', 'b1', 'parts2', 'lp1', 'lp2'):           # the refused calls touched nothing they read
        assert torch.equal(st[k], keep[k]), k
