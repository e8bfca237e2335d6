"""gd_row_nll_f32 (csrc/linkpred.hip), the loss stage of the fused node-classification step, against torch in fp64 on the same
inputs: F.nll_loss(F.log_softmax(z[:, :d_valid], 1)[rows], y[rows]) and its autograd gradient.  Bounds: the kernel suites'
(TOL of tests/test_edgeprob_kernels_gpu.py and tests/test_linkpred_kernels_gpu.py): the loss within 1e-5
relative, dz on the listed rows within 1e-5 rel-L2.  Everything else is exact: unlisted rows of dz and the columns behind
d_valid are zero, the pitch columns are untouched, two calls give equal bits, refusals launch nothing.

Every lane-group size (d = 4 ... 256), class counts d, d - 1, 3, 2 and 1, 1 ... 1000 listed rows out of 1,500 in shuffled order,
pitched z and dz, rows with logits of +-80, more rows than one sweep of the capped grid, a label out of range.
A row whose label holds nearly all of the probability has a term and gradient entries far below one ulp of its logits (the one
listed row of d = 8, 3 classes: loss 9.4e-8 from logits of 66 and 50): the bounds hold there too, which lse - z_y and
softmax_y - 1 in fp32 cannot do.

Measured on an MI355X (largest rel. distance to fp64 over the cases; the bound is TOL = 1e-5): loss 3e-7, dz rel-L2 3e-7."""
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5                                   # tests/test_edgeprob_kernels_gpu.py: TOL
N = 1500
GD_E_DIM, GD_E_ALIGN = 2, 3
SENTINEL = 12345.0


def _L():
    from gnndelete_amd import _lib
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _inputs(n, d, n_sel, seed, big_every=5):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, d, generator=g) * 2.0
    z[::big_every] = (torch.rand(z[::big_every].shape, generator=g) * 2 - 1) * 80.0        # logits up to +-80
    rows = torch.randperm(n, generator=g)[:n_sel]                                           # unique, shuffled
    return z, rows, g


def _fp64(z, rows, y, d_valid, coef=1.0):
    """(loss, dz [n, d]) in fp64; a listed row whose label is outside [0, d_valid) adds nothing and gets a zero row, but counts."""
    zz = z.double().clone().requires_grad_(True)
    lab = y[rows]
    ok = (lab >= 0) & (lab < d_valid)
    logp = F.log_softmax(zz[:, :d_valid], 1)[rows]
    terms = -logp[ok, lab[ok]]
    loss = terms.sum() / rows.numel()
    (coef * loss).backward()
    return float(loss.detach()), zz.grad


def _run(z, rows, y, d_valid, coef=1.0, ld_z=None, ld_dz=None):
    """The raw entry on pitched buffers -> (loss [1], dz view [n, d], the whole dz buffer)."""
    L = _L()
    n, d = z.shape
    ld_z, ld_dz = ld_z or d + 4, ld_dz or d + 8
    zb = torch.full((n, ld_z), float('nan'), device='cuda')
    zb[:, :d] = z.cuda()
    dzb = torch.full((n, ld_dz), SENTINEL, device='cuda')
    dzb[:, :d] = 0
    rows_c, y_c = rows.to('cuda', torch.int32), y.to('cuda', torch.int64)
    loss = torch.full((1,), SENTINEL, device='cuda')
    ws = torch.empty(max(1, L.gd_row_nll_workspace(rows.numel(), d)), device='cuda')
    rc = L.gd_row_nll_f32(zb.data_ptr(), ld_z, n, d, d_valid, rows_c.data_ptr(), rows.numel(), y_c.data_ptr(), coef, dzb.data_ptr(),
                          ld_dz, loss.data_ptr(), ws.data_ptr(), _st())
    assert rc == 0, L.gd_last_error_string()
    torch.cuda.synchronize()
    return loss, dzb[:, :d], dzb


def _check(tag, z, rows, y, d_valid, coef=1.0):
    n, d = z.shape
    want_loss, want_dz = _fp64(z, rows, y, d_valid, coef)
    loss, dz, dzb = _run(z, rows, y, d_valid, coef)
    loss2, dz2, _ = _run(z, rows, y, d_valid, coef)
    assert torch.equal(loss, loss2) and torch.equal(dz, dz2)                              # two calls: equal bits
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dz).all())
    dz_h = dz.cpu()
    listed = torch.zeros(n, dtype=torch.bool)
    listed[rows] = True
    d_loss = abs(float(loss) - want_loss) / abs(want_loss) if want_loss else abs(float(loss))
    d_dz = rel_l2(dz_h[listed], want_dz[listed]) if float(want_dz.abs().max()) > 0 else float(dz_h.abs().max())
    print(f'{tag}: loss rel {d_loss:.2e}  dz rel_l2 {d_dz:.2e}')
    assert d_loss <= TOL and d_dz <= TOL
    assert not bool(dz_h[~listed].any())                                                  # unlisted rows: exactly zero
    assert not bool(dz_h[:, d_valid:].any())                                              # behind the classes: exactly zero
    assert bool((dzb[:, d:] == SENTINEL).all())                                           # the pitch: untouched
    return loss, dz


@pytest.mark.parametrize('n_sel', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('d', [4, 8, 32, 64, 128, 256])
def test_row_nll_value_and_gradient_against_fp64(d, n_sel):
    for d_valid in sorted({v for v in (d, d - 1, 3, 2, 1) if 1 <= v <= d}):
        z, rows, g = _inputs(N, d, n_sel, seed=1000 * d + 10 * n_sel + d_valid)
        y = torch.randint(0, d_valid, (N,), generator=g)
        assert float(z[rows].abs().max()) > 40 or n_sel < 8
        _check(f'd={d} d_valid={d_valid} n_sel={n_sel}', z, rows, y, d_valid, coef=1.0 if d_valid % 2 else 0.37)


def test_row_nll_wrapper_and_a_pitched_view():
    """backbone.row_nll on a contiguous z and on a column view of a wider buffer: the same bits."""
    from gnndelete_amd.backbone import row_nll
    z, rows, g = _inputs(N, 32, 700, seed=5)
    y = torch.randint(0, 7, (N,), generator=g)
    want_loss, want_dz = _fp64(z, rows, y, 7, 2.0)
    wide = torch.full((N, 72), float('nan'))
    wide[:, 32:64] = z
    a = row_nll(z.cuda(), rows.cuda(), y.cuda(), 7, coef=2.0)
    b = row_nll(wide.cuda()[:, 32:64], rows, y, 7, coef=2.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].shape == (N, 32)
    assert abs(float(a[0]) - want_loss) <= TOL * want_loss and rel_l2(a[1].cpu(), want_dz) <= TOL
    raw, dz, _ = _run(z, rows, y, 7, 2.0)
    assert torch.equal(raw, a[0]) and torch.equal(dz, a[1])                               # the pitches change no bit


def test_row_nll_past_one_sweep_of_the_capped_grid():
    """More listed rows than the capped grid covers in one sweep: blocks walk them grid-strided."""
    L = _L()
    d = 4
    cap = int(L.gd_row_nll_workspace(1 << 30, d))                                         # the builder's block cap
    per_block = 4 * 64                                                                    # d = 4: one lane per row, 4 waves
    assert 1 <= cap <= 4096 and int(L.gd_row_nll_workspace(cap * per_block, d)) == cap
    assert int(L.gd_row_nll_workspace(cap * per_block - per_block, d)) == cap - 1
    n_sel = cap * per_block + 2 * per_block + 77                                          # a third, partial sweep
    n = n_sel + 1000
    z, rows, g = _inputs(n, d, n_sel, seed=9, big_every=50)
    y = torch.randint(0, 3, (n,), generator=g)
    _check(f'{n_sel} rows, cap {cap}', z, rows, y, 3)


def test_row_nll_label_out_of_range_adds_nothing_but_counts():
    d, d_valid = 32, 7
    z, rows, g = _inputs(N, d, 300, seed=11)
    y = torch.randint(0, d_valid, (N,), generator=g)
    bad = rows[[3, 100, 299]]
    y[bad] = torch.tensor([-1, d_valid, 10 ** 12])                                        # (7 is a padding column, in the row)
    loss, dz = _check('bad labels', z, rows, y, d_valid)
    assert not bool(dz.cpu()[bad].any())
    # the same rows left out: the same sum over 297 rows, divided by 297 instead of 300
    keep = torch.tensor([i for i in range(300) if i not in (3, 100, 299)])
    loss_kept, _, _ = _run(z, rows[keep], y, d_valid)
    assert abs(float(loss) * 300 - float(loss_kept) * 297) <= 1e-5 * float(loss) * 300


def test_row_nll_refusals_launch_nothing():
    L = _L()
    n, d = 64, 8
    z = torch.randn(n, d + 4, device='cuda')
    dz = torch.full((n, d + 8), SENTINEL, device='cuda')
    rows = torch.arange(10, dtype=torch.int32, device='cuda')
    y = torch.zeros(n, dtype=torch.int64, device='cuda')
    loss = torch.full((1,), SENTINEL, device='cuda')
    ws = torch.full((16,), SENTINEL, device='cuda')

    def call(zp=None, ld_z=d + 4, d_=d, d_valid=3, n_sel=10, dzp=None, ld_dz=d + 8):
        return L.gd_row_nll_f32(zp or z.data_ptr(), ld_z, n, d_, d_valid, rows.data_ptr(), n_sel, y.data_ptr(), 1.0,
                                dzp or dz.data_ptr(), ld_dz, loss.data_ptr(), ws.data_ptr(), _st())
    assert call(n_sel=0) == GD_E_DIM and b'gd_row_nll_f32' in L.gd_last_error_string()
    assert call(d_=6) == GD_E_DIM and b'gd_row_nll_f32' in L.gd_last_error_string()
    assert call(d_=260, ld_z=264, ld_dz=264) == GD_E_DIM
    assert call(d_=0) == GD_E_DIM
    assert call(d_valid=0) == GD_E_DIM and call(d_valid=d + 1) == GD_E_DIM
    assert call(ld_z=d + 2) == GD_E_DIM and call(ld_dz=d + 2) == GD_E_DIM and call(ld_z=d - 4) == GD_E_DIM      # the pitches
    assert call(zp=z.data_ptr() + 4) == GD_E_ALIGN and call(dzp=dz.data_ptr() + 8) == GD_E_ALIGN
    assert b'gd_row_nll_f32' in L.gd_last_error_string()
    torch.cuda.synchronize()
    assert bool((dz == SENTINEL).all()) and float(loss) == SENTINEL and bool((ws == SENTINEL).all())
    assert call() == 0                                                                     # the same buffers, accepted
    torch.cuda.synchronize()
    assert float(loss) != SENTINEL and bool((dz[10:] == SENTINEL).all()) and bool((dz[:10, d:] == SENTINEL).all())
