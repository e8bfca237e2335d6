"""The plain-GAT attention kernels (csrc/gat.hip) against fp64 on the host, at hub rows, wide logits, every width of the
balanced kernels and item counts past one trip of their persistent grid (inputs, references and measures: gat_cases.py; that
the inputs are what they claim and that fp32 alone sits inside the bounds: test_gat_cases_cpu.py).

  A  ops.gat_forward_raw (gat_items_fwd_kernel + gat_fixup_fwd_kernel) on a 6,000-node graph with rows of 1 ... 5,000
     in-edges: y, rowmax, rowsum per row, widths 4 ... 1,024, six logit regimes, with and without bias, h_rows = 0
  B  ops.gat_backward_raw, one-launch groups (GD_GAT_PIECES=0) and pieces (=1): dh, da_src, da_dst per row, alpha and the
     score gradient per CSR slot from the `ade` buffer; both source-major paths
  C  the one-wave-per-row kernels (gd_gat_aggregate_f32 / gd_gat_aggregate_bwd_f32 + rank1_add2_) as the batch step calls them
  D  plans over a row subset and a row range: rows inside meet the bounds, rows outside keep their bits
  E  36,000 and 70,000 nodes: the waves' second and third visits (loop-carried descriptor and index prefetch)
  F  build_csr on the device lays the graphs out as the host layout the cases are built on

Every error is per row (per slot for alpha and the score gradient), scaled by the sum of the magnitudes the row adds up
(gat_cases.reference), and bounded by max(8 x the error of the fp32 restatement of the same formula on the host, 2^-22); rowmax by
two fp32 ulps.  No bound is taken from a kernel's output.  The features carry one sign per column (gat_cases.case), so that
|<dy, h>|, which the score-gradient scales are made of, is the sum of the magnitudes behind it.

Measured on an MI355X (pytest -s prints every figure, per case and per listed hub row).  Per section: the largest error of
the kernels and of the fp32 restatement over the section's cases, and how close a kernel figure came to its own case's bound
(`of bound`: the largest kernel / bound over the cases; rowmax in ulps, bound 2):

  A all 34 (width, regime) cases, with and without bias, h_rows = 0
                          y     rowmax     rowsum
          kernel   2.57e-06   4.75e-01   4.37e-06
            fp32   2.58e-06   4.75e-01   4.37e-06
        of bound   2.04e-01   2.37e-01   1.29e-01
  B all 34 cases x both forms, d = 64 also with the transposition pass
                      alpha         de         dh     da_src     da_dst
          kernel   1.56e-06   4.52e-07   4.66e-06   2.43e-07   1.08e-07
            fp32   1.56e-06   1.93e-06   4.66e-06   3.56e-07   7.09e-07
        of bound   1.28e-01   1.38e-01   1.30e-01   1.35e-01   1.58e-01
  C d = 20, 64, 260 x six regimes
                          y      alpha         de         dh    dh_full     da_src     da_dst
          kernel   9.93e-07   1.58e-06   8.07e-07   4.65e-06   3.67e-07   1.56e-07   3.67e-07
            fp32   9.93e-07   1.56e-06   1.09e-06   4.65e-06   4.57e-07   2.67e-07   4.57e-07
        of bound   1.39e-01   1.28e-01   2.42e-01   1.31e-01   1.97e-01   1.64e-01   1.97e-01
  D d = 64, 16 x randn, dominant_tail: rows / range / plan / plan_t / both
                          y     rowmax     rowsum      alpha         de         dh     da_src     da_dst
          kernel   1.30e-07   4.75e-01   2.04e-07   8.71e-08   2.37e-07   1.59e-06   2.15e-07   8.99e-08
            fp32   4.43e-07   4.75e-01   2.04e-07   8.52e-08   1.42e-06   1.59e-06   1.33e-06   4.68e-07
        of bound   2.04e-01   2.37e-01   1.25e-01   1.28e-01   1.44e-01   1.29e-01   1.44e-01   1.20e-01
  E 36,000 nodes, all rows
                          y     rowmax     rowsum      alpha         de         dh     da_src     da_dst
          kernel   9.49e-08   4.75e-01   1.23e-07   1.04e-07   1.61e-07   1.53e-06   1.61e-07   9.34e-08
            fp32   2.88e-07   4.75e-01   3.61e-07   1.04e-07   5.09e-07   1.53e-06   2.98e-07   2.63e-07
        of bound   1.44e-01   2.37e-01   1.08e-01   1.25e-01   1.14e-01   1.25e-01   1.52e-01   1.05e-01
  E 36,000 nodes, rows served on a second or third visit
                          y     rowmax     rowsum      alpha         de     da_dst
          kernel   9.17e-08   4.75e-01   1.22e-07   8.60e-08   1.46e-07   8.66e-08
            fp32   2.88e-07   4.75e-01   3.61e-07   1.04e-07   5.09e-07   2.63e-07
        of bound   1.36e-01   2.37e-01   1.07e-01   1.04e-01   1.04e-01   9.52e-02
  E 70,000 nodes, all rows
                          y     rowmax     rowsum      alpha         de         dh     da_src     da_dst
          kernel   1.26e-07   4.75e-01   1.18e-07   1.20e-07   1.71e-07   7.41e-07   1.45e-07   1.03e-07
            fp32   7.39e-07   4.75e-01   1.52e-06   1.20e-07   1.57e-06   1.56e-06   1.04e-06   7.86e-07
        of bound   1.63e-01   2.37e-01   8.25e-02   1.25e-01   1.22e-01   1.25e-01   1.07e-01   1.22e-01
  E 70,000 nodes, rows served on a second or third visit
                          y     rowmax     rowsum      alpha         de     da_dst
          kernel   1.26e-07   4.75e-01   1.18e-07   1.17e-07   1.71e-07   9.76e-08
            fp32   7.39e-07   4.75e-01   1.52e-06   1.20e-07   1.57e-06   7.86e-07
        of bound   1.63e-01   2.37e-01   8.25e-02   1.22e-01   1.22e-01   1.15e-01

With features of independent signs (an earlier draw of these inputs) <dy, h> cancels inside itself, and the restatement's
score gradient per slot reached 1.2e-04 of alpha (|<dy, h>| + |t|); B at d = 128 under `wide` then missed the da_dst bound at one
three-edge row (4768: kernel 1.40e-06, restatement 1.31e-07, bound 1.05e-06; dot products of -0.6 and -0.005 from 128 terms
that add up to 79 in magnitude, the kernel's 2.6e-07 off, the host's pairwise sum 1.6e-08 by the luck of a rounding).  That is
the scale not seeing what the slot adds up, which is what this measure is for - hence the signs per column.

With arithmetic-only variants of gat.hip (scratch builds, never committed), which tests of this module fail (on the kernels as they are all 145 pass):
  1  the fix-up's piece factor e^(m_p - M) forced to 1 (112 fail): all of A except `zero`, where every factor is 1 (largest y
     error 0.013 under negative, 0.09 ... 0.14 under randn, 0.33 ... 0.89 under wide and dominant_*), the h_rows = 0 test,
     D forward, E, and B / D backward through the wrong row statistics; C and F pass
  2  a group member finishing its score gradients with its own part of t (46 fail): B, D and E with GD_GAT_PIECES=0 (da_src, de
     off by 0.07 ... 0.75); everything with pieces = 1, A, C and F pass
  3  the next visit's column indices taken from the current visit (46 fail): E forward (y off by 0.62 ... 0.89) and so all of
     E; B and D with GD_GAT_PIECES=0 as well - the one-launch items' cost-balanced ranges hold 188 ... 412 light rows of the
     6,000-node graph past the first visit (gat_cases.item_tables('hub', 'onepass', d)); A, C, F and everything with pieces = 1
     on the 6,000-node graph pass
"""
import functools
import types

import pytest
import torch

import gat_cases as C

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
EDGE = ('alpha', 'de')


@functools.lru_cache(maxsize=None)
def _graph(name):
    """F: the device build has the host layout's rowptr / col, so CSR slots mean what the regimes say."""
    from gnndelete_amd.graph import build_csr
    gph, lay = C.graph(name), C.layout(name)
    gr = build_csr(gph.ei.cuda(), gph.n, 'gat')
    assert torch.equal(gr.rowptr.cpu(), lay.gr.rowptr) and torch.equal(gr.col.cpu(), lay.gr.col), name
    assert torch.equal(gr.rowptr_t.cpu(), lay.gr.rowptr_t) and torch.equal(gr.col_t.cpu(), lay.gr.col_t), name
    return gr


def _inputs(name, regime, d):
    c = C.case(name, d)
    a_src, a_dst = C.logits(name, regime)
    return types.SimpleNamespace(h=c['h'].cuda(), dy=c['dy'].cuda(), bias=c['bias'].cuda(), a_src=a_src.cuda(), a_dst=a_dst.cuda(),
                                 att=(c['att_src'].cuda(), c['att_dst'].cuda()))


def _check(tag, got, name, regime, d, bias=False, subset=False, rows=None, report=()):
    """Largest error of every tensor in `got` (over `rows` and their slots, if given) against the bound from the restatement;
    `report`: rows whose own figures are printed (they meet the same bound)."""
    errs = C.errors(got, name, regime, d, bias, subset)
    rest, bnd = C.restatement_errors(name, regime, d, subset), C.bounds(name, regime, d, subset)
    lay = C.layout(name)
    in_rows = in_slots = None
    if rows is not None:
        in_rows = torch.zeros(C.SPEC[name]['n'], dtype=torch.bool)
        in_rows[rows.cpu()] = True
        in_slots = in_rows[lay.rows]
    key = lambda k: 'y_bias' if (k == 'y' and bias) else k
    worst = {}
    for k, e in errs.items():
        sel = e if rows is None else e[in_slots if k in EDGE else in_rows]      # (rows outside a plan may be unwritten memory)
        assert bool(torch.isfinite(sel).all()), (tag, k)
        worst[k] = float(sel.max())
    print(f'[{tag}] kernel: ' + '  '.join(f'{k} {v:.2e}' for k, v in worst.items()) + '   fp32 restatement: '
          + '  '.join(f'{k} {rest[key(k)]:.2e}' for k in worst) + '   bound: ' + '  '.join(f'{k} {bnd[key(k)]:.2e}' for k in worst))
    for r in report:
        lo, hi = int(lay.gr.rowptr[r]), int(lay.gr.rowptr[r + 1])
        print(f'[{tag}]   row {r} (in {int(lay.deg[r])}, out {int(lay.out_deg[r])}): '
              + '  '.join(f'{k} {float(e[lo:hi].max() if k in EDGE else e[r]):.2e}' for k, e in errs.items()))
    for k, v in worst.items():
        assert v <= bnd[key(k)], (tag, k, v, bnd[key(k)])
    return worst


def _count_source_major(monkeypatch):
    """Which source-major path ops.gat_backward_raw takes: calls of the two entry points."""
    from gnndelete_amd import _lib
    lib, calls = _lib.lib(), []
    for name in ('gd_spmm_csr_onepass_aux_f32', 'gd_gat_transpose_edges_f32'):
        def counted(*a, _orig=getattr(lib, name), _name=name):
            calls.append(_name)
            return _orig(*a)
        monkeypatch.setattr(lib, name, counted)
    return calls


# ---------------------------------------------------------------------------------------------------------------------
# F. layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(C.SPEC))
def test_device_build_gives_the_host_layout(name):
    gr = _graph(name)
    lay = C.layout(name)
    assert gr.nnz == lay.gr.nnz and gr.plan.n_items == lay.gr.plan.n_items
    assert torch.equal(gr.plan.items.cpu(), lay.gr.plan.items) and torch.equal(gr.plan.split.cpu(), lay.gr.plan.split)
    for d in (16, 64):
        dev, host = gr.plan.onepass(d, multirow=1), lay.gr.plan.onepass(d, multirow=1)
        assert dev[1] == host[1] and torch.equal(dev[0].cpu(), host[0]) and torch.equal(dev[2].cpu(), host[2])
    # every slot of the transposed layout points at a slot of the same edge
    perm = gr.perm_t.long().cpu()
    rows_t = torch.repeat_interleave(torch.arange(gr.n), lay.out_deg)
    assert torch.equal(lay.col[perm], rows_t) and torch.equal(lay.rows[perm], gr.col_t.long().cpu())
    assert torch.equal(torch.sort(perm).values, torch.arange(gr.nnz))


# ---------------------------------------------------------------------------------------------------------------------
# A. balanced forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,regime', C.balanced_cases())
def test_balanced_forward_holds_fp64_per_row(d, regime):
    """y, rowmax and rowsum of every row, with and without bias; finite; 1 <= rowsum <= in-degree (the maximum's own term is
    exactly 1, no term exceeds it); a second call gives the same bits."""
    from gnndelete_amd import ops
    gr, x = _graph('hub'), _inputs('hub', regime, d)
    deg = C.layout('hub').deg.cuda().float()
    for bias in (None, x.bias):
        y, rowmax, rowsum = ops.gat_forward_raw(gr, x.h, x.a_src, x.a_dst, bias, C.SLOPE)
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(rowmax).all()) and bool(torch.isfinite(rowsum).all())
        _check(f'A d = {d} {regime} bias {bias is not None}', dict(y=y, rowmax=rowmax, rowsum=rowsum), 'hub', regime, d,
               bias=bias is not None, report=C.HUB_IN if bias is None else ())
        assert bool((rowsum >= 1.0).all()) and bool((rowsum <= deg).all())
        again = ops.gat_forward_raw(gr, x.h, x.a_src, x.a_dst, bias, C.SLOPE)
        assert all(torch.equal(a, b) for a, b in zip((y, rowmax, rowsum), again))
    if regime == 'zero':
        assert torch.equal(rowsum, deg) and bool((rowmax == 0).all())


@pytest.mark.parametrize('d', [8, 512])
def test_balanced_forward_with_64_bit_addressing_gives_the_same_bits(d):
    """The raw entry with h_rows = 0 (the instances without the 24-bit row offsets) under dominant_tail: the bits of the
    call with h_rows = n, which are the bits ops.gat_forward_raw gives - and those meet the bounds above."""
    from gnndelete_amd import _lib, ops
    from gnndelete_amd._lib import check, ptr, stream_ptr
    gr, x = _graph('hub'), _inputs('hub', 'dominant_tail', d)
    n, plan, lib = gr.n, gr.plan, _lib.lib()
    scratch = plan.scratch_flat('gat', lib.gd_gat_balanced_scratch(plan.n_slots, d), x.h.device)
    out = {}
    for h_rows in (n, 0):
        y, rowmax, rowsum = (torch.full(s, SENTINEL, device='cuda') for s in ((n, d), (n,), (n,)))
        check(lib.gd_gat_aggregate_balanced_f32(ptr(plan.items), plan.n_items, ptr(plan.split), plan.n_split, plan.n_slots, ptr(gr.col),
                                                ptr(x.a_src), ptr(x.a_dst), ptr(x.h), x.h.stride(0), ptr(y), y.stride(0), ptr(x.bias),
                                                ptr(rowmax), ptr(rowsum), ptr(scratch), C.SLOPE, d, gr.nnz, h_rows,
                                                stream_ptr(x.h.device)), 'gd_gat_aggregate_balanced_f32')
        out[h_rows] = (y, rowmax, rowsum)
    want = ops.gat_forward_raw(gr, x.h, x.a_src, x.a_dst, x.bias, C.SLOPE)
    for k in range(3):
        assert torch.equal(out[0][k], out[n][k]) and torch.equal(out[n][k], want[k]), k
    _check(f'A d = {d} dominant_tail h_rows = 0', dict(y=out[0][0], rowmax=out[0][1], rowsum=out[0][2]), 'hub', 'dominant_tail', d, bias=True)


# ---------------------------------------------------------------------------------------------------------------------
# B. balanced backward
# ---------------------------------------------------------------------------------------------------------------------
def _backward(gr, x, rowmax, rowsum, **kw):
    from gnndelete_amd import ops
    bufs = {}
    dh, da_src, da_dst = ops.gat_backward_raw(gr, x.h, x.a_src, x.a_dst, rowmax, rowsum, x.dy, C.SLOPE, bufs=bufs, **kw)
    ade = bufs['ade']
    return dict(dh=dh, da_src=da_src, da_dst=da_dst, alpha=ade[:, 0], de=ade[:, 1])


@pytest.mark.parametrize('pieces', ['0', '1'])
@pytest.mark.parametrize('d,regime', C.balanced_cases())
def test_balanced_backward_holds_fp64_per_row_and_per_slot(d, regime, pieces, monkeypatch):
    """dh (message path), da_src, da_dst per row, alpha and the score gradient per CSR slot (the `ade` buffer), with the hub
    rows as groups of four members (GD_GAT_PIECES=0) and as pieces with the second edge pass (=1).  d = 64 / 128 take the
    source-major aggregation without the transposition pass, every other width gd_gat_transpose_edges_f32 + the SpMM; d = 64
    runs that form too (GD_GAT_TRANSPOSE_PASS=1).  The sources of 256 / 257 / 300 / 1,000 out-edges are printed on their own."""
    from gnndelete_amd import ops
    monkeypatch.setenv('GD_GAT_PIECES', pieces)
    monkeypatch.delenv('GD_GAT_TRANSPOSE_PASS', raising=False)
    gr, x = _graph('hub'), _inputs('hub', regime, d)
    _, rowmax, rowsum = ops.gat_forward_raw(gr, x.h, x.a_src, x.a_dst, None, C.SLOPE)
    calls = _count_source_major(monkeypatch)
    got = _backward(gr, x, rowmax, rowsum)
    assert calls == (['gd_spmm_csr_onepass_aux_f32'] if d in (64, 128) else ['gd_gat_transpose_edges_f32']), calls
    tag = f'B d = {d} {regime} pieces {pieces}'
    _check(tag, got, 'hub', regime, d, report=list(C.HUB_OUT) + [1000, 1100, 1200])
    first = {k: v.clone() for k, v in got.items()}
    again = _backward(gr, x, rowmax, rowsum)
    assert all(torch.equal(first[k], again[k]) for k in first)
    if d == 64:
        monkeypatch.setenv('GD_GAT_TRANSPOSE_PASS', '1')
        del calls[:]
        other = _backward(gr, x, rowmax, rowsum)
        assert calls == ['gd_gat_transpose_edges_f32'], calls
        _check(tag + ' with the transposition pass', other, 'hub', regime, d, report=list(C.HUB_OUT))
        assert torch.equal(other['dh'], first['dh']) and torch.equal(other['de'], first['de'])


# ---------------------------------------------------------------------------------------------------------------------
# C. the one-wave-per-row kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', C.REGIMES)
@pytest.mark.parametrize('d', C.ROW_KERNEL_WIDTHS)
def test_row_kernels_as_the_batch_step_calls_them(d, regime):
    """gd_gat_aggregate_f32 -> (y, alpha), gd_gat_aggregate_bwd_f32 -> (dh, da_src, da_dst, de) and ops.rank1_add2_ (the whole
    input gradient dh + da_src (x) att_src + da_dst (x) att_dst), as MinibatchNodeembStep._agg / _agg_bwd call them."""
    from gnndelete_amd import _lib, ops
    from gnndelete_amd._lib import check, ptr, stream_ptr
    gr, x = _graph('hub'), _inputs('hub', regime, d)
    n, lib, st = gr.n, _lib.lib(), stream_ptr(x.h.device)
    y = torch.empty(n, d, device='cuda')
    alpha = torch.empty(gr.nnz, device='cuda')
    check(lib.gd_gat_aggregate_f32(ptr(gr.rowptr), ptr(gr.col), ptr(x.a_src), ptr(x.a_dst), ptr(x.h), x.h.stride(0), ptr(y), y.stride(0),
                                   ptr(x.bias), ptr(alpha), C.SLOPE, n, d, st), 'gd_gat_aggregate_f32')
    dh = torch.empty(n, d, device='cuda')
    da = torch.empty(2, n, device='cuda')
    de = torch.empty(gr.nnz, device='cuda')
    check(lib.gd_gat_aggregate_bwd_f32(ptr(gr.rowptr), ptr(gr.col), ptr(alpha), ptr(gr.rowptr_t), ptr(gr.col_t), ptr(gr.perm_t),
                                       ptr(x.a_src), ptr(x.a_dst), ptr(x.h), x.h.stride(0), ptr(x.dy), x.dy.stride(0), ptr(dh),
                                       dh.stride(0), ptr(da[0]), ptr(da[1]), ptr(de), C.SLOPE, n, d, st), 'gd_gat_aggregate_bwd_f32')
    got = dict(y=y, alpha=alpha, de=de, dh=dh.clone(), da_src=da[0], da_dst=da[1])
    got['dh_full'] = ops.rank1_add2_(dh, da[0], x.att[0], da[1], x.att[1])
    _check(f'C d = {d} {regime}', got, 'hub', regime, d, bias=True, report=[1200, 1600])


# ---------------------------------------------------------------------------------------------------------------------
# D. row subsets
# ---------------------------------------------------------------------------------------------------------------------
def _outside(n, rows):
    m = torch.ones(n, dtype=torch.bool, device='cuda')
    m[rows] = False
    return m


@pytest.mark.parametrize('regime', ['randn', 'dominant_tail'])
@pytest.mark.parametrize('d', C.SUBSET_WIDTHS)
def test_forward_over_a_row_subset_and_a_row_range(d, regime):
    """plan=SplitPlan(rowptr, rows=...) and row_range=(400, 1001): rows inside meet the bounds, y / rowmax / rowsum of the rows
    outside keep the sentinel's bits."""
    from gnndelete_amd import ops
    from gnndelete_amd.graph import SplitPlan
    gr, x = _graph('hub'), _inputs('hub', regime, d)
    n = gr.n
    lo, hi = C.SUBSET_RANGE
    for tag, rows, plan in (('rows', C.row_subset('hub').cuda(), None), ('range', torch.arange(lo, hi).cuda(), (lo, hi))):
        plan = SplitPlan(gr.rowptr, rows=rows) if plan is None else SplitPlan(gr.rowptr, row_range=plan)
        assert plan.n_split >= 3 and plan.n_items < gr.plan.n_items
        y = torch.full((n, d), SENTINEL, device='cuda')
        bufs = {'rowmax': torch.full((n,), SENTINEL, device='cuda'), 'rowsum': torch.full((n,), SENTINEL, device='cuda')}
        out = ops.gat_forward_raw(gr, x.h, x.a_src, x.a_dst, x.bias, C.SLOPE, out=y, plan=plan, bufs=bufs)
        assert out[0] is y and out[1] is bufs['rowmax'] and out[2] is bufs['rowsum']
        _check(f'D forward {tag} d = {d} {regime}', dict(y=y, rowmax=out[1], rowsum=out[2]), 'hub', regime, d, bias=True, rows=rows,
               report=[400, 1000])
        outside = _outside(n, rows)
        assert int(outside.sum()) == n - rows.numel()
        for t in (y, out[1], out[2]):
            assert bool((t[outside] == SENTINEL).all()) and not bool((t[rows] == SENTINEL).any())


@pytest.mark.parametrize('pieces', ['0', '1'])
@pytest.mark.parametrize('regime', ['randn', 'dominant_tail'])
@pytest.mark.parametrize('d', C.SUBSET_WIDTHS)
def test_backward_over_row_subsets(d, regime, pieces, monkeypatch):
    """plan= (target rows): the slots of rows outside stay (0, 0) in `ade`, dh and da_src are the sums over the rows inside
    (reference: the upstream gradient zeroed outside).  plan_t= (source rows): dh and da_src of the rows inside meet the
    bounds, da_src outside is exactly 0.  Both together, as the engines pass them."""
    from gnndelete_amd import ops
    from gnndelete_amd.graph import SplitPlan
    monkeypatch.setenv('GD_GAT_PIECES', pieces)
    monkeypatch.delenv('GD_GAT_TRANSPOSE_PASS', raising=False)
    gr, x = _graph('hub'), _inputs('hub', regime, d)
    n = gr.n
    rows = C.row_subset('hub').cuda()
    outside = _outside(n, rows)
    slots_out = outside[C.layout('hub').rows.cuda()]
    plan, plan_t = SplitPlan(gr.rowptr, rows=rows), SplitPlan(gr.rowptr_t, rows=rows)
    assert plan.n_split >= 3 and plan_t.n_split >= 2
    _, rowmax, rowsum = ops.gat_forward_raw(gr, x.h, x.a_src, x.a_dst, None, C.SLOPE)
    tag = f'D backward d = {d} {regime} pieces {pieces}'
    # target rows
    got = _backward(gr, x, rowmax, rowsum, plan=plan)
    assert float(torch.stack([got['alpha'], got['de']])[:, slots_out].abs().max()) == 0.0
    _check(tag + ' plan', {k: got[k] for k in ('dh', 'da_src')}, 'hub', regime, d, subset=True, report=[1400, 1600])
    _check(tag + ' plan, rows inside', {k: got[k] for k in ('da_dst', 'alpha', 'de')}, 'hub', regime, d, subset=True, rows=rows,
           report=[400, 1200])
    # source rows
    got = _backward(gr, x, rowmax, rowsum, plan_t=plan_t)
    assert float(got['da_src'][outside].abs().max()) == 0.0
    _check(tag + ' plan_t', {k: got[k] for k in ('da_dst', 'alpha', 'de')}, 'hub', regime, d)
    _check(tag + ' plan_t, rows inside', {k: got[k] for k in ('dh', 'da_src')}, 'hub', regime, d, rows=rows, report=[1400, 1600])
    # both
    got = _backward(gr, x, rowmax, rowsum, plan=plan, plan_t=plan_t)
    assert float(got['da_src'][outside].abs().max()) == 0.0
    assert float(torch.stack([got['alpha'], got['de']])[:, slots_out].abs().max()) == 0.0
    _check(tag + ' plan + plan_t, rows inside', got, 'hub', regime, d, subset=True, rows=rows)


# ---------------------------------------------------------------------------------------------------------------------
# E. second and third visits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ['randn', 'dominant_tail'])
@pytest.mark.parametrize('d', C.VISIT_WIDTHS)
@pytest.mark.parametrize('name', ['visit36k', 'visit70k'])
def test_rows_served_on_a_second_or_third_visit(name, d, regime, monkeypatch):
    """Forward and backward (groups and pieces) over all rows, and over the rows whose items a wave serves on a second or later
    visit of its loop - the visits whose descriptor and column indices were fetched one and two visits earlier."""
    from gnndelete_amd import ops
    monkeypatch.delenv('GD_GAT_TRANSPOSE_PASS', raising=False)
    gr, x = _graph(name), _inputs(name, regime, d)
    hubs = list(C.SPEC[name]['hub_in'])
    later = {form: C.later_visit_rows(name, form, d) for form in ('pieces', 'onepass')}
    assert all(v.numel() > 300 for v in later.values())
    y, rowmax, rowsum = ops.gat_forward_raw(gr, x.h, x.a_src, x.a_dst, x.bias, C.SLOPE)
    fwd = dict(y=y, rowmax=rowmax, rowsum=rowsum)
    tag = f'E {name} d = {d} {regime}'
    _check(tag + ' forward', fwd, name, regime, d, bias=True, report=hubs)
    _check(tag + ' forward, later visits', fwd, name, regime, d, bias=True, rows=later['pieces'])
    for pieces in ('0', '1'):
        monkeypatch.setenv('GD_GAT_PIECES', pieces)
        got = _backward(gr, x, rowmax, rowsum)
        _check(tag + f' backward pieces {pieces}', got, name, regime, d, report=hubs)
        _check(tag + f' backward pieces {pieces}, later visits', {k: got[k] for k in ('da_dst', 'alpha', 'de')}, name, regime, d,
               rows=later['pieces' if pieces == '1' else 'onepass'])
