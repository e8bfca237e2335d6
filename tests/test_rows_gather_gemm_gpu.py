"""gd_rows_gather_gemm_f32 (ops.rows_gather_gemm): out[s] = act(x[idx[s]]) W^T (+ bias) into a compact matrix, against the
LDS-operand row GEMM on the gathered copy of the rows - the same bits - over matrix-core and odd widths, row pitches wider
than the width, id lists in any order and with repeats; what it must leave untouched; ids outside the matrix; aliasing."""
import itertools

import pytest
import torch

from gnndelete_amd import _lib, ops

pytestmark = pytest.mark.gpu

N_IN = 300
N_SEL = (0, 1, 31, 33, 200)
DIMS = [(10, 32), (32, 32), (128, 128), (128, 64), (36, 20)]
SENTINEL = -12345.5


def _pitched(rows, d, pitch, g, fill=None):
    """A [rows, d] view of a [rows, pitch] buffer: random (fill None) or a constant."""
    buf = torch.randn(rows, pitch, generator=g) if fill is None else torch.full((rows, pitch), fill)
    buf = buf.cuda()
    return buf, buf[:, :d]


def _ids(kind, n_sel, g):
    if kind == 'ascending':
        return torch.randperm(N_IN, generator=g)[:n_sel].sort().values
    if kind == 'shuffled':
        return torch.randperm(N_IN, generator=g)[:n_sel]
    ids = torch.randint(0, N_IN, (n_sel,), generator=g)
    if n_sel > 2:
        ids[-1] = ids[0]                                    # at least one repeated id
    return ids


def _reference(x, idx, w, bias, relu_in):
    return ops.rows_gemm(x.index_select(0, idx).contiguous(), None, w, trans_w=True, bias=bias, relu_in=relu_in)


@pytest.mark.parametrize('d_in,d_out', DIMS)
def test_equals_the_row_gemm_on_the_gathered_copy_and_writes_nothing_else(d_in, d_out):
    g = torch.Generator().manual_seed(1000 * d_in + d_out)
    w = torch.randn(d_out, d_in, generator=g).cuda()
    bias_v = torch.randn(d_out, generator=g).cuda()
    pitch4 = (d_in + 3) // 4 * 4
    xs = [_pitched(N_IN, d_in, p, g)[1] for p in (pitch4, pitch4 + 8)]
    checked = 0
    for n_sel, x, ld_out, kind, bias, relu_in in itertools.product(N_SEL, xs, (d_out, d_out + 8),
                                                                   ('ascending', 'shuffled', 'repeats'), (None, bias_v),
                                                                   (False, True)):
        idx = _ids(kind, n_sel, g).cuda()
        buf, _ = _pitched(n_sel + 3, d_out, ld_out, g, fill=SENTINEL)
        out = buf[:n_sel, :d_out]
        got = ops.rows_gather_gemm(x, idx, w, bias=bias, relu_in=relu_in, out=out)
        assert got is out
        tag = (n_sel, x.stride(0), ld_out, kind, bias is not None, relu_in)
        if n_sel:
            assert torch.equal(out, _reference(x, idx, w, bias, relu_in)), tag
        assert bool((buf[n_sel:] == SENTINEL).all()), tag                       # behind row n_sel
        assert bool((buf[:, d_out:] == SENTINEL).all()), tag                    # behind column d_out
        checked += 1
    assert checked == 5 * 2 * 2 * 3 * 2 * 2


@pytest.mark.parametrize('d_in,d_out', DIMS)
@pytest.mark.parametrize('with_bias', [False, True])
def test_ids_outside_the_matrix_give_zero_rows_and_leave_their_neighbours_exact(d_in, d_out, with_bias):
    g = torch.Generator().manual_seed(7 + d_in)
    w = torch.randn(d_out, d_in, generator=g).cuda()
    bias = torch.randn(d_out, generator=g).cuda() if with_bias else None
    # the matrix is the middle of a larger buffer of NaN: a read outside it poisons the result
    pitch = (d_in + 3) // 4 * 4
    big = torch.full((N_IN + 2, pitch), float('nan')).cuda()
    big[1:N_IN + 1] = torch.randn(N_IN, pitch, generator=g).cuda()
    x = big[1:N_IN + 1, :d_in]
    idx = torch.randint(0, N_IN, (70,), generator=g)
    bad = [0, 5, 31, 32, 33, 69]
    idx[bad] = torch.tensor([N_IN, -1, -1, N_IN, N_IN + 1000, -(1 << 40)])
    idx = idx.cuda()
    got = ops.rows_gather_gemm(x, idx, w, bias=bias)
    want = _reference(x, idx.clamp(0, N_IN - 1), w, bias, False)
    want[bad] = bias if with_bias else 0.0
    assert torch.equal(got, want)
    assert bool((got[bad] == (bias if with_bias else torch.zeros(d_out, device='cuda'))).all())


def test_in_place_is_refused_and_nothing_selected_is_no_launch():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64, 32, generator=g).cuda()
    w = torch.randn(32, 32, generator=g).cuda()
    before = x.clone()
    with pytest.raises(_lib.GnnDeleteHipError, match='alias'):
        ops.rows_gather_gemm(x, torch.arange(64).cuda(), w, out=x)
    assert torch.equal(x, before)
    empty = ops.rows_gather_gemm(x, torch.zeros(0, dtype=torch.int64).cuda(), w)
    assert tuple(empty.shape) == (0, 32)
    with pytest.raises(TypeError):
        ops.rows_gather_gemm(x, torch.arange(4, dtype=torch.int32).cuda(), w)
