"""gd_rows_gemm_select_chain_f32 called directly: conv2's Linear over a layer-1 output that exists on the LISTED rows only (z), the
EXPLICIT rows formed from a = A^ x in the same launch (h = a W1^T + b1 -> pre1, out = relu(h) W2^T on the first product's accumulators).

65,541 rows in all (the smallest size the weight-stationary form covers, a last unit of five live rows), 128 -> 128 -> 64, a random
interleaving of the two lists.  Explicit counts: 1 (one unit of fifteen clamped duplicates; at row 0 and at the last row), 4,101
(16 k + 5; 61,440 listed rows = a multiple of 16; 257 explicit units: most waves get none), 40,000 (more explicit than listed units)
and 60,000 (347 listed units: most waves get no listed unit); 0 explicit rows: the coverage query says no.  All four pitches wider
than the widths (a 132, z 136, out 68, pre1 132) with sentinel padding, and tight pitches once.  About half of h and of z negative,
b1 != 0, a few explicit rows whose whole h is negative (their out row is exactly zero).  The index buffers carry 16 entries BEHIND
their length that name rows of NaNs: a loop that read past the end instead of clamping would show them.

Bars.  Listed rows: bit-equal to ops.rows_gemm_select (the parent's launch) on the same inputs - the same instructions per row,
whatever unit a row falls in.  Explicit rows, out and pre1: rel-L2 error to the fp64 restatement relu(a W1^T + b1) W2^T at most
twice the error of the parent's two launches (ops.rows_gemm with the bias, then ops.rows_gemm_select) on the same inputs - the
factor covers re-association (the second product runs its k in the accumulators' feature order).  The same call twice: the same bits.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N, D, H, O = 65541, 128, 128, 64
SENTINEL = 7.5
PITCHES = dict(a=132, z=136, out=68, pre=132)
N_NEG = 3                                    # explicit rows whose whole h is negative (cases with more than 100 explicit rows)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@functools.lru_cache(maxsize=None)
def _base():
    """Inputs shared by every case, built once, never modified: N live rows + 2 rows of NaNs nobody lists."""
    g = torch.Generator(device='cuda').manual_seed(4100)

    def randn(*shape):
        return torch.randn(*shape, device='cuda', generator=g)
    a, z = randn(N + 2, D), randn(N + 2, H)
    a[N:], z[N:] = float('nan'), float('nan')
    w1 = (randn(H, D) / D ** 0.5).contiguous()                 # Linear weights: [out, in], dense and not symmetric
    w2 = (randn(O, H) / H ** 0.5).contiguous()
    b1 = (0.3 * randn(H)).contiguous()
    # an input row whose conv1 output is -3 - |noise| in every column
    neg_a = torch.linalg.solve(w1.double(), (-3.0 - randn(N_NEG, H).abs().double() - b1.double()).t()).t().float().contiguous()
    perm = torch.randperm(N, device='cuda', generator=g)
    return dict(a=a, z=z, w1=w1, w2=w2, b1=b1, neg_a=neg_a, perm=perm)


def _pitched(t, pitch):
    buf = torch.full((t.shape[0], pitch), SENTINEL, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf, buf[:, :t.shape[1]]


@functools.lru_cache(maxsize=None)
def _case(n_expl, where='random'):
    """One partition of the N rows into explicit and listed rows, its inputs, the parent's two launches and the fp64 restatement."""
    from gnndelete_amd import ops
    b = _base()
    if where == 'first':
        expl = torch.zeros(1, dtype=torch.long, device='cuda')
    elif where == 'last':
        expl = torch.full((1,), N - 1, dtype=torch.long, device='cuda')
    else:
        expl = torch.sort(b['perm'][:n_expl]).values
    assert expl.numel() == n_expl
    mask = torch.zeros(N + 2, dtype=torch.bool, device='cuda')
    mask[expl] = True
    listed = (~mask[:N]).nonzero().flatten()
    a = b['a'].clone()
    neg_rows = expl[:0]
    if n_expl > 100:
        neg_rows = expl[torch.tensor([0, n_expl // 2, n_expl - 1], device='cuda')]      # first, middle and last explicit row
        a[neg_rows] = b['neg_a']
    nan_ids = torch.tensor([N, N + 1] * 8, dtype=torch.int32, device='cuda')
    idx_e = torch.cat([expl.to(torch.int32), nan_ids]).contiguous()[:n_expl]
    idx_l = torch.cat([listed.to(torch.int32), nan_ids]).contiguous()[:listed.numel()]
    # the parent's two launches (tight buffers; the selector names the listed rows)
    sel = (~mask).to(torch.uint8).contiguous()
    sel[N:] = 0
    pre_ref = torch.zeros(N + 2, H, device='cuda')
    ops.rows_gemm(a, idx_e, b['w1'], trans_w=True, const_w=True, bias=b['b1'], out=pre_ref)
    out_ref = torch.zeros(N + 2, O, device='cuda')
    ops.rows_gemm_select(pre_ref, b['z'], sel, b['w2'], trans_w=True, const_w=True, relu_in=True, out=out_ref, idx=torch.arange(N, dtype=torch.int32, device='cuda'))
    out_sel = ops.rows_gemm_select(pre_ref[:N], b['z'][:N], sel[:N].contiguous(), b['w2'], trans_w=True, const_w=True, relu_in=True)
    h64 = a[expl].double() @ b['w1'].double().t() + b['b1'].double()
    out64 = h64.clamp(min=0) @ b['w2'].double().t()
    torch.cuda.synchronize()
    return dict(a=a, expl=expl, listed=listed, idx_e=idx_e, idx_l=idx_l, neg_rows=neg_rows, pre_ref=pre_ref, out_ref=out_ref, out_sel=out_sel,
                h64=h64, out64=out64)


def _call(c, pitched):
    from gnndelete_amd import ops
    b = _base()
    bufs = {}
    if pitched:
        bufs['a'], a = _pitched(c['a'], PITCHES['a'])
        bufs['z'], z = _pitched(b['z'], PITCHES['z'])
        bufs['out'], out = _pitched(torch.full((N + 2, O), -1.0, device='cuda'), PITCHES['out'])
        bufs['pre'], pre = _pitched(torch.zeros(N + 2, H, device='cuda'), PITCHES['pre'])
    else:
        a, z = c['a'], b['z']
        out, pre = torch.full((N + 2, O), -1.0, device='cuda'), torch.zeros(N + 2, H, device='cuda')
    got = ops.rows_gemm_select_chain(a, c['idx_e'], b['w1'], b['b1'], pre, z, c['idx_l'], b['w2'], out=out)
    assert got is out
    torch.cuda.synchronize()
    return out, pre, bufs


CASES = [(1, 'first', True), (1, 'last', True), (4101, 'random', True), (4101, 'random', False), (40000, 'random', True),
         (60000, 'random', True)]


@pytest.mark.parametrize('n_expl,where,pitched', CASES)
def test_chained_select_product(n_expl, where, pitched):
    from gnndelete_amd import ops
    c = _case(n_expl, where)
    n_list = N - n_expl
    assert ops.rows_gemm_select_chain_ok(n_list, n_expl, D, H, O)
    assert (n_list % 16 == 0) == (n_expl == 4101)
    out, pre, bufs = _call(c, pitched)
    expl, listed = c['expl'], c['listed']
    # the inputs are about half negative, and the all-negative rows are what they claim to be
    assert 0.4 < float((_base()['z'][:N] < 0).double().mean()) < 0.6
    if n_expl > 100:
        assert 0.4 < float((c['h64'] < 0).double().mean()) < 0.6
        pos = torch.searchsorted(expl, c['neg_rows'])
        assert bool((c['h64'][pos] < -2.9).all()) and float(c['out64'][pos].abs().max()) == 0.0
        assert float(out[c['neg_rows']].abs().max()) == 0.0 and bool((pre[c['neg_rows']] < 0).all())
    # listed rows: the parent's launch, bit for bit (dense and as an index list over the same rows); pre1 untouched there
    assert torch.equal(out[listed], c['out_sel'][listed]) and torch.equal(out[listed], c['out_ref'][listed])
    assert float(pre[listed].abs().max()) == 0.0
    # the NaN rows behind the lists were neither read into a result nor written
    assert bool(torch.isfinite(out[:N]).all()) and bool(torch.isfinite(pre[:N]).all())
    assert float((out[N:] + 1.0).abs().max()) == 0.0 and float(pre[N:].abs().max()) == 0.0
    # explicit rows against fp64, held to twice the parent's two launches
    e_pre, e_pre_par = _rel(pre[expl], c['h64']), _rel(c['pre_ref'][expl], c['h64'])
    e_out, e_out_par = _rel(out[expl], c['out64']), _rel(c['out_ref'][expl], c['out64'])
    print(f'[explicit chain kernel] MEASURED n_expl={n_expl} ({where}, pitched={pitched}) to fp64: pre1 {e_pre:.2e} (parent {e_pre_par:.2e}), '
          f'out {e_out:.2e} (parent {e_out_par:.2e})')
    assert e_pre <= 2.0 * e_pre_par and e_out <= 2.0 * e_out_par
    # padding columns keep their sentinel
    for name, buf in bufs.items():
        width = {'a': D, 'z': H, 'out': O, 'pre': H}[name]
        assert buf.shape[1] == PITCHES[name] and float((buf[:, width:] - SENTINEL).abs().max()) == 0.0, name
    # the same call twice gives the same bits
    out2, pre2, _ = _call(c, pitched)
    assert torch.equal(out2[:N], out[:N]) and torch.equal(pre2[:N], pre[:N])


def test_coverage_query_and_refusals():
    from gnndelete_amd import ops
    from gnndelete_amd._lib import GnnDeleteHipError
    assert not ops.rows_gemm_select_chain_ok(N, 0, D, H, O)            # no explicit rows: the parent's selector product is the step
    assert ops.rows_gemm_select_chain_ok(65535, 1, D, H, O) and not ops.rows_gemm_select_chain_ok(65534, 1, D, H, O)
    assert ops.rows_gemm_select_chain_ok(0, 65536, D, H, O)
    for widths in ((64, 128, 64), (128, 64, 64), (128, 128, 128), (128, 128, 32)):
        assert not ops.rows_gemm_select_chain_ok(N - 5, 5, *widths), widths
    b, c = _base(), _case(4101)
    with pytest.raises(GnnDeleteHipError):                             # below the row range: an error, no other form behind the call
        ops.rows_gemm_select_chain(c['a'], c['idx_e'][:5], b['w1'], b['b1'], torch.zeros(N + 2, H, device='cuda'), b['z'], c['idx_l'][:100], b['w2'])
