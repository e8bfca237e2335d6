"""The R-GAT attention path on the HIP kernels against fp64 on the host, at hub rows, wide logits and node counts past one
sweep of a grid (inputs: rgat_cases.py; the fp32 oracle's own distances to fp64: test_rgat_cases_cpu.py).

  A  gd_segment_softmax_f32 / gd_segment_softmax_bwd_f32: rows of 0, 1, 63, 64, 65, 128, 129, 1,000, 5,000 and 2 entries,
     logits that are randn, +-150, 3e4 + randn, all equal, or led by entries 60 above the rest
  B  RGATConv on a 2,000-node knowledge graph with a 1,500-edge hub target and a 1,000-edge hub source: the no-grad kernel
     branch, the typed-conv branch and the typed_weighted_sum + einsum branch, gradients to x, weight, q, k and bias
  C  gd_rgcn_conv_f32 with per-edge coefficients on 65,545 nodes (the grid sweeps 65,536 rows and strides)
  D  gd_rowpair_dot_f32 at every lane-group width, pitched rows and an unaligned base
  E  the two-layer RGATDelete, every parameter trainable

Measured on an MI355X (pytest -s prints every figure; the host's fp32 figures move in the last digit with its thread count).

A, all 12 rows (the 1-, 4- and 5-row prefixes give no larger figure); largest per-element error to fp64, de scaled by its
row's max |dalpha|; the bound is max(8 x restatement, 2^-22 = 2.38e-07):

    regime     kernel: alpha   de        row sum     fp32 restatement: alpha   de        row sum     bound: alpha   de
    randn              2.60e-08  1.46e-08  6.00e-08                      2.60e-08  2.28e-08  1.99e-06           2.38e-07  2.38e-07
    wide               4.42e-08  1.49e-08  4.62e-08                      4.42e-08  1.98e-08  4.62e-08           3.54e-07  2.38e-07
    offset             1.81e-08  5.65e-09  8.37e-08                      2.48e-08  6.84e-09  9.71e-07           2.38e-07  2.38e-07
    equal              9.17e-10  8.18e-09  5.77e-08                      9.17e-10  8.18e-09  5.77e-08           2.38e-07  2.38e-07
    dominant           4.16e-08  7.69e-08  1.12e-07                      4.16e-08  5.65e-08  1.25e-07           3.33e-07  4.52e-07

   (the restatement's own row sums drift by 2e-6 over the 5,000-entry row: index_add adds one by one.  The kernel's
   lanes-then-wave order does not, and fp32 with pairwise row sums stays below 9.5e-08: test_rgat_cases_cpu.py.)
   With the first or the second loop of segment_softmax_fwd_kernel cut to a single trip, or `- m` dropped, this test fails:
   max loop -> wide (exp overflows past entry 64); sum loop -> every regime (rows above 64 entries sum past 1);
   no `- m` -> wide, offset (exp(3e4) = inf) and equal.

B, rel-L2 to fp64 on the hub graph (bounds 1e-5 on y, 2e-5 on the gradients):

    shape (in, out, blocks)     y         dx        dweight   dq        dk        dbias     row 17 of y  row 23 of dx  no_grad y
    128, 64, 4      kernels     1.52e-07  8.12e-07  8.48e-07  1.20e-06  9.50e-07  1.26e-07  3.90e-07     5.19e-07      1.52e-07
                    fp32 oracle 1.84e-07  1.13e-06  1.25e-06  1.67e-06  1.92e-06  1.07e-07
    64, 128, 4      kernels     1.12e-07  8.90e-07  9.10e-07  1.01e-06  1.14e-06  1.03e-07  1.57e-07     1.04e-06      1.12e-07
    16, 8, None     kernels     4.39e-08  2.16e-07  4.44e-07  4.56e-07  3.32e-07  9.10e-08  5.37e-08     3.33e-07      4.39e-08
    12, 12, 4       kernels     3.70e-08  1.36e-07  2.24e-07  2.93e-07  3.20e-07  7.45e-08  2.02e-08     2.24e-07      3.70e-08
    132, 8, None    kernels     1.76e-07  4.87e-07  4.90e-07  9.66e-07  4.58e-07  6.13e-08  6.04e-07     5.44e-07      1.76e-07
    wide logits (128, 64, 4 with 4 q, 4 k: fp64 logit span 221.0; gradient bound max(2e-5, 3 x fp32 oracle)):
                    kernels     2.76e-07  4.28e-06  4.19e-06  4.83e-06  3.86e-06  1.26e-07  1.02e-07     3.67e-06      2.76e-07
                    fp32 oracle 3.50e-07  4.26e-06  4.18e-06  5.20e-06  4.40e-06  1.07e-07

C, n = 65,545: every figure (y, dx, dweight, dcoef; rows >= 65,536 and rows < 11 on their own) at most 5.8e-07 (bound 2e-5).
E: z1, z2 at most 2.6e-07 (bound 1e-5), every gradient at most 1.5e-06 (bound 2e-5).
"""
import collections

import pytest
import torch

import rgat_cases as C
from helpers import hip_model, rel_l2

pytestmark = pytest.mark.gpu
SENTINEL = 777.0


# ---------------------------------------------------------------------------------------------------------------------
# A. segment softmax
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', C.REGIMES)
def test_segment_softmax_kernels_hold_fp64_at_every_row_length(regime):
    """alpha and de per element against fp64 autograd of pyg.segment_softmax.  Bound: 8 x the error of the fp32 restatement
    of the same formula on the host (another summation order, the fast exponential's |x| 2^-24 exponent rounding), floor
    2^-22 - measured from the reference, never from the kernel.  Rows sum to 1 within it, the result is finite, a second
    launch (the raw entry, into a buffer with a sentinel tail) gives the same bits and leaves the tail alone."""
    from gnndelete_amd import _lib, ops
    lib = _lib.lib()
    for n_rows in C.PREFIXES:
        rowptr = C.softmax_rowptr(n_rows)
        nnz = int(rowptr[-1])
        rowptr_d = rowptr.cuda()
        e = C.softmax_logits(regime)[:nnz].cuda().requires_grad_()
        up = C.softmax_upstream()[:nnz].cuda()
        alpha = ops.segment_softmax(e, rowptr_d)
        alpha.backward(up)
        de = e.grad
        assert alpha.shape == (nnz,) and de.shape == (nnz,)
        assert bool(torch.isfinite(alpha).all()) and bool(torch.isfinite(de).all())
        ka, kd, ks = C.softmax_errors(alpha.detach().cpu(), de.cpu(), regime, n_rows)
        ra, rd, rs = C.softmax_restatement_errors(regime, n_rows)
        ba, bd = C.softmax_bounds(regime, n_rows)
        print(f'[softmax {regime:8s} rows {n_rows:2d}] kernel: alpha {ka:.2e}  de {kd:.2e}  row sum {ks:.2e}   '
              f'fp32 restatement: alpha {ra:.2e}  de {rd:.2e}  row sum {rs:.2e}   bounds {ba:.2e} / {bd:.2e}')
        assert ka <= ba, (regime, n_rows, ka, ba)
        assert kd <= bd, (regime, n_rows, kd, bd)
        assert ks <= ba, (regime, n_rows, ks, ba)
        if nnz == 0:
            continue
        # the raw entries once more, into buffers with a sentinel tail
        ec = e.detach().contiguous()
        a_buf = torch.full((nnz + 67,), SENTINEL, device='cuda')
        d_buf = torch.full((nnz + 67,), SENTINEL, device='cuda')
        stream = _lib.stream_ptr(ec.device)
        _lib.check(lib.gd_segment_softmax_f32(rowptr_d.data_ptr(), ec.data_ptr(), n_rows, a_buf.data_ptr(), stream), 'gd_segment_softmax_f32')
        _lib.check(lib.gd_segment_softmax_bwd_f32(rowptr_d.data_ptr(), a_buf.data_ptr(), up.data_ptr(), n_rows, d_buf.data_ptr(), stream),
                   'gd_segment_softmax_bwd_f32')
        assert torch.equal(a_buf[:nnz], alpha.detach()) and torch.equal(d_buf[:nnz], de)
        assert bool((a_buf[nnz:] == SENTINEL).all()) and bool((d_buf[nnz:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
# B. RGATConv on the hub graph
# ---------------------------------------------------------------------------------------------------------------------
def _conv(d_in, d_out, nb, wide):
    from gnndelete_amd import nn as gnn
    c = C.layer_case(d_in, d_out, nb, wide)
    conv = gnn.RGATConv(d_in, d_out, C.N_REL, num_blocks=nb)
    with torch.no_grad():
        for name in ('weight', 'q', 'k', 'bias'):
            getattr(conv, name).copy_(c[name])
    return conv.cuda(), c


def _forward_backward(conv, c, ei, et):
    x = c['x'].cuda().requires_grad_()
    conv.zero_grad(set_to_none=True)
    y = conv(x, ei, et)
    y.backward(c['gy'].cuda())
    out = {'y': y.detach(), 'dx': x.grad}
    out.update({'d' + n: getattr(conv, n).grad.clone() for n in ('weight', 'q', 'k', 'bias')})
    return out


def _count_branches(monkeypatch):
    from gnndelete_amd import ops
    calls = collections.Counter()
    for name in ('typed_conv', 'typed_weighted_sum', 'rgat_aggregate_nograd'):
        def counted(*a, _orig=getattr(ops, name), _name=name, **kw):
            calls[_name] += 1
            return _orig(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    return calls


@pytest.mark.parametrize('d_in,d_out,nb,wide', [s + (False,) for s in C.KERNEL_SHAPES + C.FALLBACK_SHAPES] + [C.WIDE_SHAPE + (True,)])
def test_rgat_conv_matches_the_fp64_oracle_on_the_hub_graph(d_in, d_out, nb, wide, monkeypatch):
    """Every branch of RGATConv.forward against pyg.rgat_conv in fp64: y at 1e-5, the gradients to x, weight, q, k and bias
    at 2e-5 (wide logits: max(2e-5, 3 x the fp32 oracle's own distance)), the 1,500-edge row of y and the 1,000-edge row of
    dx on their own, rows without in-edges = the bias, the relation without edges = a zero weight gradient, same bits twice."""
    kernel_shape = (d_in, d_out, nb) in C.KERNEL_SHAPES
    ei, et = (t.cuda() for t in C.hub_graph())
    conv, c = _conv(d_in, d_out, nb, wide)
    ref = C.layer_reference_fp64(d_in, d_out, nb, wide)
    d32 = C.layer_fp32_distances(d_in, d_out, nb, wide)
    if wide:
        assert ref['span'] > C.WIDE_MIN_SPAN
    calls = _count_branches(monkeypatch)
    got = _forward_backward(conv, c, ei, et)
    assert dict(calls) == ({'typed_conv': 1} if kernel_shape else {'typed_weighted_sum': 1}), calls
    dist = {n: rel_l2(got[n].cpu(), ref[n]) for n in got}
    tag = f'rgat_conv {d_in}->{d_out} blocks {nb}' + (' wide logits' if wide else '')
    print(f'[{tag}] logit span {ref["span"]:.1f}; kernels to fp64: ' + '  '.join(f'{k} {v:.2e}' for k, v in dist.items()))
    print(f'[{tag}] fp32 oracle to fp64: ' + '  '.join(f'{k} {v:.2e}' for k, v in d32.items()))
    assert dist['y'] < C.TOL, dist
    for n in C.GRAD_NAMES:
        bound = max(C.GRAD_TOL, 3 * d32['d' + n]) if wide else C.GRAD_TOL
        assert dist['d' + n] < bound, (n, dist['d' + n], bound)
    hub_y = rel_l2(got['y'][C.HUB_IN].cpu(), ref['y'][C.HUB_IN])
    hub_dx = rel_l2(got['dx'][C.HUB_OUT].cpu(), ref['dx'][C.HUB_OUT])
    print(f'[{tag}] row {C.HUB_IN} of y {hub_y:.2e}  row {C.HUB_OUT} of dx {hub_dx:.2e}')
    assert hub_y < C.TOL and hub_dx < C.GRAD_TOL
    iso = slice(C.N_NODES - C.N_ISOLATED, C.N_NODES)
    bias_rows = c['bias'].cuda().expand(C.N_ISOLATED, -1)
    assert torch.equal(got['y'][iso], bias_rows)
    assert float(got['dweight'][-1].abs().max()) == 0.0 and float(got['dweight'][0].abs().max()) > 0
    # the same forward under no_grad: the fused kernel branch for even block widths up to 128
    calls.clear()
    with torch.no_grad():
        y_ng = conv(c['x'].cuda(), ei, et)
        y_ng2 = conv(c['x'].cuda(), ei, et)
    assert dict(calls) == ({'rgat_aggregate_nograd': 2} if kernel_shape else {'typed_weighted_sum': 2}), calls
    d_ng = rel_l2(y_ng.cpu(), ref['y'])
    print(f'[{tag}] no_grad forward to fp64: {d_ng:.2e}')
    assert d_ng < C.TOL and rel_l2(y_ng[C.HUB_IN].cpu(), ref['y'][C.HUB_IN]) < C.TOL
    assert torch.equal(y_ng[iso], bias_rows) and torch.equal(y_ng, y_ng2)
    again = _forward_backward(conv, c, ei, et)
    for n in got:
        assert torch.equal(again[n], got[n]), n


# ---------------------------------------------------------------------------------------------------------------------
# C. the node-major typed conv past one sweep of its grid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d_in,d_out,nb', C.LARGE_SHAPES)
def test_typed_conv_with_coefficients_past_one_grid_sweep(d_in, d_out, nb, monkeypatch):
    """ops.typed_conv with per-edge coefficients (gd_rgcn_conv_f32 forward and, transposed with bwd_order, for the input
    gradient) on 65,545 nodes: the waves that own rows 0 ... 8 come back for rows 65,536 ... 65,544."""
    from gnndelete_amd import _lib, ops
    from gnndelete_amd.graph import TypedNodeCSR
    ei, et = C.large_graph()
    c = C.large_case(d_in, d_out, nb)
    ref = C.large_reference_fp64(d_in, d_out, nb)
    launches = []
    lib = _lib.lib()
    orig = lib.gd_rgcn_conv_f32
    monkeypatch.setattr(lib, 'gd_rgcn_conv_f32', lambda *a: (launches.append(a[10]), orig(*a))[1])       # (a[10] = trans)
    tg = TypedNodeCSR(ei.cuda(), et.cuda(), C.LARGE_N, C.LARGE_REL)
    blocks = nb or 1
    wk = (c['weight'] if nb else c['weight'].view(C.LARGE_REL, d_in, d_out)).cuda().requires_grad_()
    xk, ck = c['x'].cuda().requires_grad_(), c['coef'].cuda().requires_grad_()
    y = ops.typed_conv(xk, tg, wk, blocks, ck)
    y.backward(c['gy'].cuda())
    assert launches == [0, 1], launches
    got = dict(y=y.detach(), dx=xk.grad, dweight=wk.grad.view_as(c['weight']), dcoef=ck.grad)
    dist = {n: rel_l2(got[n].cpu(), ref[n]) for n in got}
    second = {n: rel_l2(got[n][C.SWEEP:].cpu(), ref[n][C.SWEEP:]) for n in ('y', 'dx')}
    first = {n: rel_l2(got[n][:11].cpu(), ref[n][:11]) for n in ('y', 'dx')}
    print(f'[typed conv n = {C.LARGE_N} {d_in}->{d_out} blocks {nb}] kernels to fp64: ' + '  '.join(f'{k} {v:.2e}' for k, v in dist.items())
          + f'   rows >= {C.SWEEP}: y {second["y"]:.2e} dx {second["dx"]:.2e}   rows < 11: y {first["y"]:.2e} dx {first["dx"]:.2e}')
    assert max(dist.values()) < C.GRAD_TOL, dist
    assert max(second.values()) < C.GRAD_TOL and max(first.values()) < C.GRAD_TOL, (second, first)
    assert float(got['dweight'][-1].abs().max()) == 0.0
    untouched = torch.ones(C.LARGE_N, dtype=torch.bool)
    untouched[ei[1]] = False
    assert float(got['y'][untouched.cuda()].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# D. row-pair dot products
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [4, 16, 20, 64, 68, 256, 260, 10])
def test_rowpair_dot_at_every_lane_group_width_and_layout(d):
    """gd_rowpair_dot_f32 through the C ABI: out[k] = <a[ia[k]], b[ib[k]]> with 4, 8, 16, 32 and 64 lanes per pair (d / 4 <= lanes),
    the one-wave-per-pair kernel for d = 260, d = 10 and a base that is not 16-byte aligned; contiguous rows and rows at a pitch
    of d + 4; repeated and out-of-order indices; 1, 65 and 1,000 pairs (one lane group, a partial last block, many blocks)."""
    from gnndelete_amd import _lib
    lib = _lib.lib()
    g = torch.Generator().manual_seed(900 + d)
    rows_a, rows_b = 37, 53
    for layout in ('contiguous', 'pitched', 'unaligned'):
        ld = d + 4 if layout == 'pitched' else d
        off = 1 if layout == 'unaligned' else 0
        buf_a, buf_b = torch.randn(rows_a * ld + 4, generator=g), torch.randn(rows_b * ld + 4, generator=g)
        dev_a, dev_b = buf_a.cuda(), buf_b.cuda()
        a = dev_a[off:off + rows_a * ld].view(rows_a, ld)
        b = dev_b[off:off + rows_b * ld].view(rows_b, ld)
        assert a.data_ptr() % 16 == 4 * off and b.data_ptr() % 16 == 4 * off
        a64 = buf_a[off:off + rows_a * ld].view(rows_a, ld)[:, :d].double()
        b64 = buf_b[off:off + rows_b * ld].view(rows_b, ld)[:, :d].double()
        for n in (1, 65, 1000):
            ia, ib = torch.randint(0, rows_a, (n,), generator=g), torch.randint(0, rows_b, (n,), generator=g)
            if n > 1:
                ia[-1], ib[-1] = ia[0], ib[0]                                     # a repeated pair, far apart
                assert int(ia.unique().numel()) < n and bool((ia[1:] < ia[:-1]).any())
            want = (a64[ia] * b64[ib]).sum(1)
            out = torch.full((n + 9,), SENTINEL, device='cuda')
            ia_d, ib_d = ia.to(torch.int32).cuda(), ib.to(torch.int32).cuda()
            _lib.check(lib.gd_rowpair_dot_f32(a.data_ptr(), ld, ia_d.data_ptr(), b.data_ptr(), ld, ib_d.data_ptr(), n, d, out.data_ptr(),
                                              _lib.stream_ptr(out.device)), 'gd_rowpair_dot_f32')
            err = rel_l2(out[:n].cpu(), want)
            assert err < C.TOL, (d, layout, n, err)
            assert bool((out[n:] == SENTINEL).all()), (d, layout, n)
            assert torch.equal(out[n - 1], out[0]) or n == 1


# ---------------------------------------------------------------------------------------------------------------------
# E. two-layer RGATDelete
# ---------------------------------------------------------------------------------------------------------------------
def test_two_layer_rgat_delete_with_every_parameter_trainable():
    """RGATDelete and the fp64 oracle from one seeded state on the hub graph, masks over both hubs and rows without in-edges.
    The Del forward freezes conv1 (no_grad kernel branch) and trains through conv2: z1, z2, both Del weights and conv2's
    weight, q, k and bias.  The backbone forward (what the backbone trainer runs) reaches conv1 and the node embedding."""
    state, mask1, mask2, u1, u2 = C.model_case()
    ref = C.model_reference_fp64()
    ei, et = (t.cuda() for t in C.hub_graph())
    x = torch.arange(C.N_NODES).cuda()
    for tag in ('del', 'backbone'):
        m = hip_model('rgat', state, mask1, mask2, num_nodes=C.N_NODES, num_edge_type=C.MODEL_EDGE_TYPES)
        assert all(p.requires_grad for p in m.parameters())
        z1, z2 = (m(x, ei, et, return_all_emb=True) if tag == 'del' else m.get_original_embeddings(x, ei, et, return_all_emb=True))
        ((z1 * u1.cuda()).sum() + (z2 * u2.cuda()).sum()).backward()
        dist = {'z1': rel_l2(z1.detach().cpu(), ref[tag]['z1']), 'z2': rel_l2(z2.detach().cpu(), ref[tag]['z2'])}
        params = dict(m.named_parameters())
        for n, want in ref[tag]['grads'].items():
            if want is None:
                assert params[n].grad is None, (tag, n)
            else:
                dist[n] = rel_l2(params[n].grad.cpu(), want)
        print(f'[two-layer RGATDelete, {tag} forward] kernels to fp64: ' + '  '.join(f'{k} {v:.2e}' for k, v in dist.items()))
        assert len(dist) == (2 + 6 if tag == 'del' else 2 + 9), dist
        for k, v in dist.items():
            assert v < (C.TOL if k in ('z1', 'z2') else C.GRAD_TOL), (tag, k, v)
        for z, want in ((z1, ref[tag]['z1']), (z2, ref[tag]['z2'])):
            for row in (C.HUB_IN, C.HUB_OUT, C.N_NODES - 7, C.N_NODES - 1):
                assert rel_l2(z[row].detach().cpu(), want[row]) < C.TOL, (tag, row)
