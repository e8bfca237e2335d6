"""The C ABI called with row pitches WIDER than the width, against fp64 closed forms.

The engines run GraphSAGE on column halves of double-width buffers and the mini-batch step works in static buffers, so the
entries are handed views whose pitch is not their width; the kernel suite (test_kernels_gpu.py) passes contiguous tensors
almost everywhere.  Here every matrix argument of an entry is a view [:, off:off + d] of a [rows, d + pad] buffer:

    (off, pad) = (0, 4)   four spare columns (the smallest pitch the float4 paths accept);
                 (0, d)   the left half of a double-width buffer;
                 (d, d)   the right half: the base pointer is not at the start of an allocation's row;

and the arguments of one call get DIFFERENT layouts (argument k of the call takes layout (k + r) mod 3; r = 0, 1, 2).
Input pad columns hold NaN (a read outside the view poisons the result); outputs are pre-filled with a sentinel that must
survive bit for bit in the pad columns and in the rows the call does not list.  Per call: (a) the fp64 closed form at
test_kernels_gpu.py's bound for that entry (no new tolerance), (b) the sentinel, (c) the same bits as the same call on
contiguous copies.  (c) is asserted for EVERY case of this file: every layout keeps 16-byte aligned rows and pitches that are
multiples of 4 and no buffer reaches 4 GiB, and on the device no entry was met that picks another kernel form, or another
summation order, for a pitched call of these sizes - so no case carries an exemption.  An entry that one day legitimately
dispatches by pitch must say so at its case and keep (a) and (b).

Adding an entry = one function call(P) that takes its matrices from a `_Pitched` and returns its outputs, run by _all_layouts
(the row GEMM modes: one line in ROWS_MODES)."""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import random_graph, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5                                   # tests/test_kernels_gpu.py
SENTINEL = -777.25
LAYOUTS = [(0, 4), (0, 'd'), ('d', 'd')]
BIG = 70_003                                 # rows of the shared inputs above the 65,536-row threshold of the weight-stationary forms


def _L():
    from gnndelete_amd import _lib
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what=''):
    from gnndelete_amd import _lib
    _lib.check(rc, what)


def _p(t):
    return None if t is None else t.data_ptr()


class _Pitched:
    """Hands out the matrix arguments of ONE call.  rot = None: contiguous; else argument k gets LAYOUTS[(k + rot) % 3]."""

    def __init__(self, rot):
        self.rot, self.k, self.last, self.outs = rot, 0, None, []

    def _layout(self, d, same):
        if self.rot is None:
            return 0, 0
        if not same:
            off, pad = LAYOUTS[(self.k + self.rot) % 3]
            self.k += 1
            self.last = (off, pad)
        off, pad = self.last
        return (d if off == 'd' else off), (d if pad == 'd' else pad)

    def inp(self, t, same=False):
        """A pitched copy of the [rows, d] matrix t (NaN around it).  same = the layout of the previous argument (for entries
        that take ONE pitch for two matrices)."""
        rows, d = t.shape
        off, pad = self._layout(d, same)
        buf = torch.full((rows, d + pad), float('nan'), device='cuda')
        buf[:, off:off + d] = t
        v = buf[:, off:off + d]
        assert v.data_ptr() % 16 == 0 and v.stride(0) % 4 == 0 and v.stride(0) == d + pad
        return v

    def halves(self, a, b):
        """a and b as the two halves of one double-width buffer (GraphSAGE's t2 = [x W_l | x W_r])."""
        rows, d = a.shape
        if self.rot is None:
            return a.contiguous(), b.contiguous()
        self.k += 1
        if self.rot == 0:
            buf = torch.cat([a, b], 1).contiguous()
            return buf[:, :d], buf[:, d:]
        if self.rot == 1:
            buf = torch.cat([b, a], 1).contiguous()
            return buf[:, d:], buf[:, :d]
        buf = torch.full((rows, 2 * d + 8), float('nan'), device='cuda')       # [a | 4 NaN | b | 4 NaN]: pitch 2 d + 8
        buf[:, :d], buf[:, d + 4:2 * d + 4] = a, b
        return buf[:, :d], buf[:, d + 4:2 * d + 4]

    def out(self, rows, d, init=None, same=False):
        """A sentinel-filled output (the view holds `init` where the entry accumulates or leaves rows alone)."""
        off, pad = self._layout(d, same)
        buf = torch.full((max(rows, 1), d + pad), SENTINEL, device='cuda')
        if init is not None:
            buf[:, off:off + d] = init
        v = buf[:, off:off + d]
        self.outs.append((buf, off, d, v))
        return v

    def assert_pads_intact(self):
        for buf, off, d, _ in self.outs:
            keep = torch.ones(buf.shape[1], dtype=torch.bool, device='cuda')
            keep[off:off + d] = False
            assert bool((buf[:, keep] == SENTINEL).all()), 'a pad column of an output was written'


def _assert_rows_untouched(v, rows_written, init=None):
    rest = torch.ones(v.shape[0], dtype=torch.bool, device='cuda')
    if rows_written is not None:
        rest[rows_written.long()] = False
    else:
        rest[:] = False
    got = v[rest]
    assert bool((got == SENTINEL).all()) if init is None else torch.equal(got, init[rest]), 'a row outside the index list was written'


def _all_layouts(call):
    """call(P) -> dict of outputs; it asserts (a) and the untouched rows itself.  (b) pads and (c) bit equality here."""
    base = {k: v.clone() for k, v in call(_Pitched(None)).items()}
    for rot in range(3):
        P = _Pitched(rot)
        got = call(P)
        P.assert_pads_intact()
        for k, v in got.items():
            assert torch.equal(v, base[k]), f'layout rotation {rot}: {k} differs from the contiguous call, max |diff| ' \
                                            f'{float((v.double() - base[k].double()).abs().nan_to_num(nan=float("inf")).max()):.3e}'


def _close(got, want, tol=TOL):
    e = rel_l2(got.double().cpu(), want.double().cpu())
    assert e < tol, e


def _sums_close(lp, want):
    np.testing.assert_allclose(lp.reshape(-1, 2).double().sum(0).cpu().numpy(), [float(w) for w in want], rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------------ shared inputs

@pytest.fixture(scope='module', autouse=True)
def _drop_shared_inputs():
    """The >= 65,536-row inputs and the hub graph are shared by the cases of this module and released with it."""
    yield
    for f in (_rows_data, _loss_data, _hub_graph, _gat_graph, _typed_graph):
        f.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=2)
def _rows_data(n, d_in, d_out):
    g = torch.Generator(device='cuda').manual_seed(n + 7 * d_in + d_out)
    r = lambda *s: torch.randn(*s, generator=g, device='cuda')
    D = dict(n=n, d_in=d_in, d_out=d_out, x=r(n, d_in), x2=r(n, d_in), w=r(d_in, d_out) * 0.2, bias=r(d_out), base=r(n, d_out),
             u1=r(d_out), u2=r(d_out), ra=r(n), rb=r(n))
    mask = torch.rand(n, generator=g, device='cuda') < 0.95
    mask[-1] = True
    if int(mask.sum()) % 16 == 0:
        mask[int(mask.nonzero()[0])] = False
    D['idx'] = mask.nonzero().flatten().int()
    s = D['idx'].numel()
    assert s % 16 != 0 and (n < 65_536 or s >= 65_536)
    D['sel'] = (torch.rand(n, generator=g, device='cuda') < 0.4).to(torch.uint8)
    D['bits'] = torch.randint(-2 ** 31, 2 ** 31, (s, (d_out + 31) // 32), generator=g, device='cuda', dtype=torch.int64).int()
    D['gate'] = (((D['bits'][:, :, None] >> torch.arange(32, dtype=torch.int32, device='cuda')) & 1).reshape(s, -1)[:, :d_out]).bool()
    D['wt'] = D['w'].t().contiguous()
    D['want'] = D['x'].double() @ D['w'].double()
    D['want_relu'] = D['x'].double().clamp(min=0) @ D['w'].double()
    return D


def _unpack(bits, d):
    return (((bits[:, :, None] >> torch.arange(32, dtype=torch.int32, device=bits.device)) & 1).reshape(bits.shape[0], -1)[:, :d]).bool()


# ------------------------------------------------------------------------------------------------ row GEMM family

def _rg_plain(P, D, use_idx=True, trans_w=0, bias=False, relu=0, save=False):
    n, di, do = D['n'], D['d_in'], D['d_out']
    idx = D['idx'] if use_idx else None
    s = idx.numel() if use_idx else n
    x = P.inp(D['x'])
    out = P.out(n, do)
    sv = torch.full((s, di), SENTINEL, device='cuda') if save else None          # (compact by contract: the entry takes no pitch for it)
    _ok(_L().gd_rows_gemm_f32(_p(x), x.stride(0), _p(idx), s, _p(D['wt'] if trans_w else D['w']), di, do, trans_w, _p(D['bias']) if bias else None,
                              relu, _p(out), out.stride(0), _p(sv), _st()), 'gd_rows_gemm_f32')
    li = idx.long() if use_idx else torch.arange(n, device='cuda')
    want = (D['want_relu'] if relu else D['want'])[li] + (D['bias'].double() if bias else 0.0)
    _close(out[li], want)
    _assert_rows_untouched(out, idx)
    res = dict(out=out[li])
    if save:
        assert torch.equal(sv, D['x'][li])
        res['save'] = sv
    return res


def _rg_signs(P, D):
    n, di, do = D['n'], D['d_in'], D['d_out']
    idx, li = D['idx'], D['idx'].long()
    x = P.inp(D['x'])
    out = P.out(n, do)
    bits = torch.zeros_like(D['bits'])
    _ok(_L().gd_rows_gemm_signs_f32(_p(x), x.stride(0), _p(idx), idx.numel(), _p(D['w']), di, do, 0, None, 0, _p(out), out.stride(0), None,
                                    _p(bits), _st()), 'gd_rows_gemm_signs_f32')
    _close(out[li], D['want'][li])
    _assert_rows_untouched(out, idx)
    assert torch.equal(_unpack(bits, do), out[li] > 0)
    return dict(out=out[li], bits=bits)


def _rg_gated(P, D, rank1=False):
    n, di, do = D['n'], D['d_in'], D['d_out']
    idx, li = D['idx'], D['idx'].long()
    x = P.inp(D['x'])
    out = P.out(n, do)
    L = _L()
    if rank1:
        _ok(L.gd_rows_gemm_gated_rank1_f32(_p(x), x.stride(0), _p(idx), idx.numel(), _p(D['w']), di, do, 0, _p(D['bits']), _p(D['ra']), _p(D['u1']),
                                           _p(D['rb']), _p(D['u2']), _p(out), out.stride(0), _st()), 'gd_rows_gemm_gated_rank1_f32')
        want = D['want'] + D['ra'].double()[:, None] * D['u1'].double() + D['rb'].double()[:, None] * D['u2'].double()
    else:
        _ok(L.gd_rows_gemm_gated_f32(_p(x), x.stride(0), _p(idx), idx.numel(), _p(D['w']), di, do, 0, _p(D['bits']), _p(out), out.stride(0), _st()),
            'gd_rows_gemm_gated_f32')
        want = D['want']
    _close(out[li], want[li] * D['gate'])
    assert bool((out[li][~D['gate']] == 0).all())
    _assert_rows_untouched(out, idx)
    return dict(out=out[li])


def _rg_select(P, D, use_idx=True):
    n, di, do = D['n'], D['d_in'], D['d_out']
    idx = D['idx'] if use_idx else None
    li = idx.long() if use_idx else torch.arange(n, device='cuda')
    x = P.inp(D['x'])
    x2 = P.inp(D['x2'], same=True)                   # one ld_in for both buffers
    out = P.out(n, do)
    _ok(_L().gd_rows_gemm_select_f32(_p(x), _p(x2), _p(D['sel']), x.stride(0), _p(idx), li.numel(), _p(D['w']), di, do, 0, _p(D['bias']), 1,
                                     _p(out), out.stride(0), _st()), 'gd_rows_gemm_select_f32')
    want = torch.where(D['sel'].bool()[:, None], D['x2'].double(), D['x'].double()).clamp(min=0) @ D['w'].double() + D['bias'].double()
    _close(out[li], want[li])
    _assert_rows_untouched(out, idx)
    return dict(out=out[li])


def _rg_accumulate(P, D, use_idx=True, trans_w=0):
    n, di, do = D['n'], D['d_in'], D['d_out']
    idx = D['idx'] if use_idx else None
    li = idx.long() if use_idx else torch.arange(n, device='cuda')
    L = _L()
    x = P.inp(D['x'])
    out = P.out(n, do, init=D['base'])
    rc = L.gd_rows_gemm_accumulate_f32(_p(x), x.stride(0), _p(idx), li.numel(), _p(D['wt'] if trans_w else D['w']), di, do, trans_w, _p(out),
                                       out.stride(0), _st())
    if not L.gd_rows_gemm_ws_covers(li.numel(), di, do):
        # no other form exists below the threshold / off the weight-stationary widths: refused (the header says so), nothing written
        assert rc == 2 and b'gd_rows_gemm_accumulate_f32' in L.gd_last_error_string()
        assert torch.equal(out, D['base'])
        return dict(out=out[li])
    _ok(rc, 'gd_rows_gemm_accumulate_f32')
    _close(out[li], D['base'].double()[li] + D['want'][li])
    _assert_rows_untouched(out, idx, init=D['base'])
    return dict(out=out[li])


def _rg_dots(P, D, use_idx=True, select=False):
    n, di, do = D['n'], D['d_in'], D['d_out']
    idx = D['idx'] if use_idx else None
    li = idx.long() if use_idx else torch.arange(n, device='cuda')
    x = P.inp(D['x'])
    x2 = P.inp(D['x2'], same=True) if select else None
    out = P.out(n, do)
    o1, o2 = torch.full((n,), SENTINEL, device='cuda'), torch.full((n,), SENTINEL, device='cuda')
    _ok(_L().gd_rows_gemm_dots_f32(_p(x), _p(x2), _p(D['sel']) if select else None, x.stride(0), _p(D['wt']), di, do, 1, _p(D['bias']), 0, _p(out),
                                   out.stride(0), _p(idx), li.numel(), _p(D['u1']), _p(D['u2']), _p(o1), _p(o2), _st()), 'gd_rows_gemm_dots_f32')
    xin = torch.where(D['sel'].bool()[:, None], D['x2'].double(), D['x'].double()) if select else D['x'].double()
    want = xin @ D['w'].double() + D['bias'].double()
    _close(out[li], want[li])
    _close(o1[li], want[li] @ D['u1'].double())
    _close(o2[li], want[li] @ D['u2'].double())
    _assert_rows_untouched(out, idx)
    _assert_rows_untouched(o1[:, None], idx)
    _assert_rows_untouched(o2[:, None], idx)
    return dict(out=out[li], o1=o1[li], o2=o2[li])


ROWS_MODES = {
    'plain-idx': lambda P, D: _rg_plain(P, D),
    'plain-dense-transw-relu': lambda P, D: _rg_plain(P, D, use_idx=False, trans_w=1, relu=1),
    'plain-idx-bias-relu': lambda P, D: _rg_plain(P, D, bias=True, relu=1),
    'plain-idx-save': lambda P, D: _rg_plain(P, D, save=True),
    'signs': _rg_signs,
    'gated': _rg_gated,
    'select-idx': _rg_select,
    'select-dense': lambda P, D: _rg_select(P, D, use_idx=False),
    'accumulate-idx-transw': lambda P, D: _rg_accumulate(P, D, trans_w=1),
    'accumulate-dense': lambda P, D: _rg_accumulate(P, D, use_idx=False),
}
MFMA_ONLY_MODES = {                                   # entries without a generic-width form
    'gated-rank1': lambda P, D: _rg_gated(P, D, rank1=True),
    'dots-idx': _rg_dots,
    'dots-dense-select': lambda P, D: _rg_dots(P, D, use_idx=False, select=True),
}
MFMA_WIDTHS = [(128, 128), (128, 64), (64, 128), (64, 64)]


@pytest.mark.parametrize('mode', list(ROWS_MODES) + list(MFMA_ONLY_MODES))
@pytest.mark.parametrize('d_in,d_out', MFMA_WIDTHS)
@pytest.mark.parametrize('n', [301, BIG])
def test_rows_gemm_family_pitched_mfma_widths(n, d_in, d_out, mode):
    """n = 301: the LDS-operand kernels; n = 70,003 (>= 65,536 listed rows, not a multiple of the 16-row unit): the
    weight-stationary ones where gd_rows_gemm_ws_covers says so."""
    assert _L().gd_rows_gemm_ws_covers(BIG - 4000, d_in, d_out) == (0 if os.environ.get('GD_ROWS_GEMM_WS') == '0' else 1)
    assert _L().gd_rows_gemm_ws_covers(301, d_in, d_out) == 0
    D = _rows_data(n, d_in, d_out)
    fn = {**ROWS_MODES, **MFMA_ONLY_MODES}[mode]
    _all_layouts(lambda P: fn(P, D))


@pytest.mark.parametrize('mode', list(ROWS_MODES))
@pytest.mark.parametrize('d_in,d_out', [(12, 20), (20, 12)])
def test_rows_gemm_family_pitched_generic_widths(d_in, d_out, mode):
    D = _rows_data(301, d_in, d_out)
    _all_layouts(lambda P: ROWS_MODES[mode](P, D))


@pytest.mark.parametrize('m,k,n', [(300, 1664, 128), (1000, 96, 64), (77, 8736, 128), (2500, 352, 96), (64, 32, 32)])
@pytest.mark.parametrize('use_idx', [False, True])
def test_gemm_wide_pitched(m, k, n, use_idx):
    L = _L()
    g = torch.Generator(device='cuda').manual_seed(m + k)
    x = torch.randn(m, k, generator=g, device='cuda')
    w = torch.randn(k, n, generator=g, device='cuda') * 0.1
    b = torch.randn(n, generator=g, device='cuda')
    idx = (torch.rand(m, generator=g, device='cuda') < 0.7).nonzero().flatten().int() if use_idx else None
    li = idx.long() if use_idx else torch.arange(m, device='cuda')
    want = x.double() @ w.double() + b.double()
    ws = torch.empty(max(1, L.gd_gemm_f32_workspace(li.numel(), k, n)), device='cuda')

    def call(P):
        xv = P.inp(x)
        out = P.out(m, n)
        _ok(L.gd_gemm_f32(_p(xv), xv.stride(0), _p(idx), li.numel(), _p(w), k, n, _p(b), _p(out), out.stride(0), _p(ws), _st()), 'gd_gemm_f32')
        _close(out[li], want[li])
        _assert_rows_untouched(out, idx)
        return dict(out=out[li])
    _all_layouts(call)


# ------------------------------------------------------------------------------------------------ weight gradients

@functools.lru_cache(maxsize=2)
def _loss_data(n, d, seed=0, d_p=None):
    """Rows, index list, loss slots (some rows without one), folded targets - the inputs of the fused loss entries."""
    g = torch.Generator(device='cuda').manual_seed(n + d + seed)
    r = lambda *s: torch.randn(*s, generator=g, device='cuda')
    D = dict(n=n, d=d, p=r(n, d_p or d), z=r(n, d), add=r(n, d) * 0.1, w=torch.eye(d, device='cuda') + 0.05 * r(d, d))
    mask = torch.rand(n, generator=g, device='cuda') < 0.95
    mask[-1] = True
    if int(mask.sum()) % 16 == 0:
        mask[int(mask.nonzero()[0])] = False
    idx = mask.nonzero().flatten()
    s = idx.numel()
    has = torch.rand(s, generator=g, device='cuda') < 0.8
    n_slots = int(has.sum())
    slot = torch.full((s,), -1, dtype=torch.int32, device='cuda')
    slot[has] = torch.randperm(n_slots, generator=g, device='cuda').int()
    D.update(idx=idx.int(), s=s, has=has, slot=slot, tm=r(n_slots, d), coef=torch.rand(n_slots, generator=g, device='cuda') + 0.1,
             cnt=torch.randint(1, 4, (n_slots,), generator=g, device='cuda').float()
             * torch.where(torch.rand(n_slots, generator=g, device='cuda') < 0.5, -1.0, 1.0))
    return D


def _loss_terms(D, z64):
    """g = coef_u (z - tm_u) on the rows with a slot (else 0) and the two loss sums, fp64; z64 = the selected rows' z."""
    sl = D['slot'][D['has']].long()
    df = z64[D['has']] - D['tm'].double()[sl]
    gm = torch.zeros_like(z64)
    gm[D['has']] = D['coef'].double()[sl][:, None] * df
    sq = (df * df).sum(1) * D['cnt'].double()[sl].abs()
    return gm, [sq[D['cnt'][sl] >= 0].sum(), sq[D['cnt'][sl] < 0].sum()]


@pytest.mark.parametrize('n,d_a,d_b', [(300, 128, 128), (300, 64, 64), (300, 128, 64), (300, 32, 64), (50, 12, 20), (BIG, 128, 64),
                                       (BIG, 128, 128), (BIG, 64, 64), (BIG, 64, 128)])
def test_wgrad_pitched(n, d_a, d_b):
    """ld_a != ld_g; relu_mask and g_add share ld_g with g.  The entry has ONE form per width pair (no row-count switch: the
    row count only sets the number of blocks and the rows each owns, 438 x 160 at 70,003 rows against 3 x 128 at 300)."""
    L = _L()
    g = torch.Generator(device='cuda').manual_seed(n + d_a)
    r = lambda *s: torch.randn(*s, generator=g, device='cuda')
    a, gr, rm, ga, base = r(n, d_a), r(n, d_b), r(n, d_b), r(n, d_b), r(d_a, d_b)
    idx = (torch.rand(n, generator=g, device='cuda') < 0.9).nonzero().flatten().int()
    li, s = idx.long(), idx.numel()
    want = base.double() + a.double()[li].t() @ (gr.double() * (rm > 0) + ga.double())[li]
    ws = torch.empty(L.gd_rows_gemm_wgrad_workspace(s, d_a, d_b), device='cuda')

    def call(P):
        av, gv = P.inp(a), P.inp(gr)
        rv, gav = P.inp(rm, same=True), P.inp(ga, same=True)
        dw = base.clone()
        _ok(L.gd_rows_gemm_wgrad_f32(_p(av), av.stride(0), _p(idx), _p(gv), gv.stride(0), _p(idx), _p(rv), _p(gav), s, d_a, d_b, _p(dw), 1, _p(ws),
                                     _st()), 'gd_rows_gemm_wgrad_f32')
        _close(dw, want)
        return dict(dw=dw)
    _all_layouts(call)


@pytest.mark.parametrize('n,d', [(3000, 128), (300, 64), (300, 32), (BIG, 128), (BIG, 64), (BIG, 32)])
def test_wgrad_loss_pitched(n, d):
    """(One form per width here too; the large cases change the block geometry only.)"""
    L = _L()
    D = _loss_data(n, d)
    li, s = D['idx'].long(), D['s']
    gm, sums = _loss_terms(D, D['z'].double()[li])
    want = D['p'].double()[li].t() @ (gm + D['add'].double()[li])
    nb = L.gd_rows_gemm_wgrad_blocks(s)

    def call(P):
        av, zv = P.inp(D['p']), P.inp(D['z'])
        addv = P.inp(D['add'], same=True)
        ws = torch.full((nb * d * d,), 3.0, device='cuda')
        lp = torch.full((2 * nb,), 5.0, device='cuda')
        _ok(L.gd_rows_gemm_wgrad_loss_f32(_p(av), av.stride(0), _p(D['idx']), _p(zv), zv.stride(0), _p(D['idx']), _p(D['slot']), _p(D['tm']),
                                          _p(D['coef']), _p(D['cnt']), _p(addv), s, d, d, None, 0, _p(ws), _p(lp), None, None, None, None,
                                          1e-3, 0.9, 0.999, 1e-8, _st()), 'gd_rows_gemm_wgrad_loss_f32')
        _close(ws.view(nb, d, d).double().sum(0), want)
        _sums_close(lp, sums)
        return dict(ws=ws, lp=lp)
    _all_layouts(call)


# ------------------------------------------------------------------------------------------------ fused Del passes

@pytest.mark.parametrize('entry', ['gd_del_loss_bwd_f32', 'gd_del_loss_bwd_wgrad_f32', 'gd_del_loss_bwd_wgrad_parts_f32'])
@pytest.mark.parametrize('n,d', [(500, 64), (300, 32), (BIG, 64), (BIG, 32)])
def test_del2_fused_pitched(n, d, entry):
    """ld_p, ld_dz, ld_dp each of its own (the SAGE engine's dp is a half of dcat: pitch 2 d).  d = 64 at >= 65,536 rows is the
    weight-stationary form of the two wgrad entries."""
    L = _L()
    D = _loss_data(n, d)
    li, s = D['idx'].long(), D['s']
    w64 = D['w'].double()
    dz_want, sums = _loss_terms(D, D['p'].double()[li] @ w64)
    dp_want = dz_want @ w64.t()
    dw_want = D['p'].double()[li].t() @ dz_want
    if entry == 'gd_del_loss_bwd_f32':
        nb = L.gd_del_loss_bwd_blocks(s)
    elif entry == 'gd_del_loss_bwd_wgrad_f32':
        nb = L.gd_rows_gemm_wgrad_blocks(s)
    else:
        nb = L.gd_del_loss_bwd_wgrad_parts(s, d)
        assert 1 <= nb <= L.gd_rows_gemm_wgrad_blocks(s)

    def call(P):
        pv = P.inp(D['p'])
        dz = P.out(s, d)
        dp = P.out(n, d)
        lp = torch.full((2 * nb,), 5.0, device='cuda')
        ws = torch.full((nb * d * d,), 3.0, device='cuda')
        head = [_p(pv), pv.stride(0), _p(D['idx']), s, _p(D['w']), d, _p(D['slot']), _p(D['tm']), _p(D['coef']), _p(D['cnt']), _p(dz), dz.stride(0),
                _p(dp), dp.stride(0), _p(lp)]
        if entry == 'gd_del_loss_bwd_f32':
            _ok(L.gd_del_loss_bwd_f32(*head, _st()), entry)
        elif entry == 'gd_del_loss_bwd_wgrad_f32':
            _ok(L.gd_del_loss_bwd_wgrad_f32(*head, _p(ws), _st()), entry)
        else:
            _ok(L.gd_del_loss_bwd_wgrad_parts_f32(*head, _p(ws), nb, _st()), entry)
        _close(dz[:s], dz_want)
        _close(dp[li], dp_want)
        _assert_rows_untouched(dp, D['idx'])
        _sums_close(lp, sums)
        res = dict(dz=dz[:s], dp=dp[li], lp=lp)
        if entry != 'gd_del_loss_bwd_f32':
            _close(ws.view(nb, d, d).double().sum(0), dw_want)
            res['ws'] = ws
        return res
    _all_layouts(call)


@pytest.mark.parametrize('n', [1000, BIG])
@pytest.mark.parametrize('chain', [False, True])
def test_del1_fused_pitched(n, chain):
    """gd_del1_loss_wgrad_f32 (ld_p, ld_z, ld_gadd) and gd_del1_chain_loss_wgrad_f32 (ld_p, ld_z, ld_dt).  d = 128 is the only
    width these two entries exist for (the header: first-layer Del at d = 128, d_next = 64); 70,003 rows is where
    gd_del1_loss_wgrad_covers holds."""
    L = _L()
    d = 128
    D = _loss_data(n, d, seed=1)
    li, s = D['idx'].long(), D['s']
    assert L.gd_del1_loss_wgrad_covers(s, d) == (1 if n == BIG and os.environ.get('GD_DEL1_FUSED') != '0' else 0)
    g = torch.Generator(device='cuda').manual_seed(n)
    dt = torch.randn(n, 64, generator=g, device='cuda') * 0.1
    w_next = torch.randn(64, d, generator=g, device='cuda') * 0.2
    sign_in = torch.randint(-2 ** 31, 2 ** 31, (s, 4), generator=g, device='cuda', dtype=torch.int64).int()
    z_want = D['p'].double()[li] @ D['w'].double()
    gm, sums = _loss_terms(D, z_want)
    if chain:
        g_add = (dt.double()[li] @ w_next.double()) * _unpack(sign_in, d)
    else:
        g_add = D['add'].double()[li]
    dw_want = D['p'].double()[li].t() @ (gm + g_add)
    nb = L.gd_del1_loss_wgrad_parts(s)
    assert 1 <= nb <= L.gd_rows_gemm_wgrad_blocks(s)

    def call(P):
        pv = P.inp(D['p'])
        z = P.out(n, d)
        third = P.inp(dt if chain else D['add'])
        bits = sign_in.clone()
        lp = torch.full((2 * nb,), 5.0, device='cuda')
        ws = torch.full((nb * d * d,), 3.0, device='cuda')
        if chain:
            _ok(L.gd_del1_chain_loss_wgrad_f32(_p(pv), pv.stride(0), _p(D['idx']), s, _p(D['w']), d, _p(z), z.stride(0), _p(bits), _p(D['slot']),
                                               _p(D['tm']), _p(D['coef']), _p(D['cnt']), _p(third), third.stride(0), 64, _p(w_next), None, None,
                                               None, None, _p(lp), _p(ws), nb, _st()), 'gd_del1_chain_loss_wgrad_f32')
        else:
            _ok(L.gd_del1_loss_wgrad_f32(_p(pv), pv.stride(0), _p(D['idx']), s, _p(D['w']), d, _p(z), z.stride(0), _p(bits), _p(D['slot']),
                                         _p(D['tm']), _p(D['coef']), _p(D['cnt']), _p(third), third.stride(0), _p(lp), _p(ws), nb, _st()),
                'gd_del1_loss_wgrad_f32')
        _close(z[li], z_want, 1e-6)                       # (the bounds of test_del1_forward_loss_and_weight_gradient_in_one_pass)
        _assert_rows_untouched(z, D['idx'])
        assert torch.equal(_unpack(bits, d), z[li] > 0)
        _close(ws.view(nb, d, d).double().sum(0), dw_want, 2e-6)
        _sums_close(lp, sums)
        return dict(z=z[li], bits=bits, ws=ws, lp=lp)
    _all_layouts(call)


# ------------------------------------------------------------------------------------------------ aggregation

@functools.lru_cache(maxsize=1)
def _hub_graph():
    from gnndelete_amd.graph import build_csr
    n = 12000
    g = torch.Generator().manual_seed(5)
    hubs = [(0, 5000), (7, 65), (11, 128), (12, 129), (4000, 257), (11999, 1000), (6000, 64)]
    star = [torch.stack([torch.randint(0, n, (k,), generator=g), torch.full((k,), h)]) for h, k in hubs]
    ei = torch.cat([random_graph(n, 40000, seed=5)] + star, 1)
    gr = build_csr(ei.cuda(), n, 'sum')
    assert gr.plan.n_split >= 6
    val = torch.rand(gr.col.shape[0], generator=g).cuda() + 0.5
    rows = torch.repeat_interleave(torch.arange(n, device='cuda'), (gr.rowptr[1:] - gr.rowptr[:-1]).long())
    av = torch.zeros(n, n, dtype=torch.float64, device='cuda').index_put_((rows, gr.col.long()), val.double(), accumulate=True)
    return n, gr, val, av


@pytest.mark.parametrize('form', ['plain', 'balanced', 'onepass', 'onepass-x_rows-0'])
@pytest.mark.parametrize('d', [128, 64, 32, 8, 260])
def test_spmm_forms_pitched(d, form, monkeypatch):
    """gd_spmm_csr_f32, the two-launch balanced form and the one-launch form (hub rows of 65 ... 5,000 in-edges), with edge
    values, bias and - the balanced forms - the self term read from the OTHER half of the buffer x lives in (GraphSAGE)."""
    from gnndelete_amd import ops
    n, gr, val, av = _hub_graph()
    g = torch.Generator(device='cuda').manual_seed(d)
    x = torch.randn(n, d, generator=g, device='cuda')
    xs = torch.randn(n, d, generator=g, device='cuda')
    b = torch.randn(d, generator=g, device='cuda')
    if form == 'balanced':
        monkeypatch.setenv('GD_SPMM_TWO_LAUNCH', '1')
    L = _L()

    def call(P):
        if form == 'plain':
            xv = P.inp(x)
            y = P.out(n, d)
            ops._spmm_raw(gr.rowptr, gr.col, val, xv, b, 0.5, n, None, out=y)
            want = av @ x.double() + 0.5 * x.double() + b.double()
        else:
            xv, xsv = P.halves(x, xs)
            y = P.out(n, d)
            if form == 'onepass-x_rows-0':                # 64-bit addressing instead of the 32-bit row offsets
                items, n_items, bounds = gr.plan.onepass(d)
                _ok(L.gd_spmm_csr_onepass_f32(_p(items), n_items, _p(gr.col), _p(val), _p(xv), xv.stride(0), _p(y), y.stride(0), _p(b), 1.0,
                                              _p(xsv), d, int(gr.col.shape[0]), 0, _p(bounds), _st()), 'gd_spmm_csr_onepass_f32')
            else:
                ops._spmm_raw(gr.rowptr, gr.col, val, xv, b, 1.0, n, gr.plan, out=y, x_self=xsv)
            want = av @ x.double() + xs.double() + b.double()
        _close(y, want)
        return dict(y=y)
    _all_layouts(call)


@pytest.mark.parametrize('d', [128, 64, 20, 4])
def test_rgcn_mean_pitched(d):
    L = _L()
    n, R, m = 300, 5, 4000
    g = torch.Generator().manual_seed(d)
    src, dst, rel = torch.randint(0, n, (m,), generator=g), torch.randint(0, n - 20, (m,), generator=g), torch.randint(0, R, (m,), generator=g)
    key = rel * n + dst
    order = torch.argsort(key, stable=True)
    rowptr = torch.zeros(R * n + 1, dtype=torch.int32)
    rowptr[1:] = torch.bincount(key, minlength=R * n).cumsum(0)
    col = src[order].int()
    x = torch.randn(n, d, generator=g)
    a = torch.zeros(R * n, n, dtype=torch.float64).index_put_((key, src), torch.ones(m, dtype=torch.float64), accumulate=True)
    want = (a / a.sum(1, keepdim=True).clamp(min=1)) @ x.double()
    rg, cg, xg = rowptr.cuda(), col.cuda(), x.cuda()

    def call(P):
        xv = P.inp(xg)
        y = P.out(R * n, d)
        _ok(L.gd_rgcn_mean_f32(_p(rg), _p(cg), _p(xv), xv.stride(0), _p(y), y.stride(0), R, n, d, _st()), 'gd_rgcn_mean_f32')
        _close(y, want)
        assert bool((y[(a.sum(1) == 0).cuda()] == 0).all())        # empty segments are written as zeros
        return dict(y=y)
    _all_layouts(call)


# ------------------------------------------------------------------------------------------------ losses and decoders

@pytest.mark.parametrize('d', [128, 64, 16, 260])
@pytest.mark.parametrize('with_dz', [True, False])
def test_rowtarget_mse_pitched(d, with_dz):
    L = _L()
    n = 700
    D = _loss_data(n, d, seed=2)
    keep = D['has']
    row_idx = D['idx'][keep]                                      # one touched row per slot ...
    order = D['slot'][keep].long()                                # ... in slot order
    rows = torch.empty_like(row_idx)
    rows[order] = row_idx
    u = rows.numel()
    kind = (D['cnt'] < 0).int()
    cnt = D['cnt'].abs()
    df = D['z'].double()[rows.long()] - D['tm'].double()
    dz_want = D['coef'].double()[:, None] * df
    sq = (df * df).sum(1) * cnt.double()
    sums_want = [float(sq[kind == 0].sum()), float(sq[kind == 1].sum())]
    ws = torch.empty(L.gd_rowtarget_mse_workspace(u), device='cuda')

    def call(P):
        zv = P.inp(D['z'])
        dz = P.out(n, d) if with_dz else None
        sums = torch.zeros(2, device='cuda')
        _ok(L.gd_rowtarget_mse_f32(_p(zv), zv.stride(0), _p(D['tm']), d, _p(rows), _p(D['coef']), _p(cnt), _p(kind), u, _p(dz),
                                   dz.stride(0) if with_dz else 0, _p(sums), _p(ws), _st()), 'gd_rowtarget_mse_f32')
        np.testing.assert_allclose(sums.double().cpu().numpy(), sums_want, rtol=1e-5)
        res = dict(sums=sums)
        if with_dz:
            _close(dz[rows.long()], dz_want)
            _assert_rows_untouched(dz, rows)
            res['dz'] = dz[rows.long()]
        return res
    _all_layouts(call)


@pytest.mark.parametrize('d', [64, 128, 12, 4])
@pytest.mark.parametrize('distmult', [False, True])
def test_edge_dot_pitched(d, distmult):
    L = _L()
    g = torch.Generator(device='cuda').manual_seed(d)
    n, m, r = 70, 333, 5
    z = torch.randn(n, d, generator=g, device='cuda')
    rel = torch.randn(r, d, generator=g, device='cuda')
    e = torch.randint(0, n, (2, m), generator=g, device='cuda')
    et = torch.randint(0, r, (m,), generator=g, device='cuda')
    want = (z.double()[e[0]] * (rel.double()[et] if distmult else 1.0) * z.double()[e[1]]).sum(-1)

    def call(P):
        zv = P.inp(z)
        rv = P.inp(rel) if distmult else None
        out = torch.full((m,), SENTINEL, device='cuda')
        _ok(L.gd_edge_dot_f32(_p(zv), zv.stride(0), d, _p(e[0].contiguous()), _p(e[1].contiguous()), _p(rv), rv.stride(0) if distmult else 0,
                              _p(et) if distmult else None, m, _p(out), _st()), 'gd_edge_dot_f32')
        _close(out, want)
        return dict(out=out)
    _all_layouts(call)


@pytest.mark.parametrize('d', [128, 64, 16, 260])
@pytest.mark.parametrize('compact', [0, 1])
def test_rowpair_mse_pitched(d, compact):
    """ld_z, ld_o, ld_dz; dz indexed by row (only touched rows written) and compact."""
    L = _L()
    g = torch.Generator().manual_seed(d)
    n, n_seg = 90, 40
    z, o = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    rows = torch.randperm(n, generator=g)[:n_seg].sort().values
    cnt = torch.randint(0, 4, (n_seg,), generator=g)
    seg_ptr = torch.zeros(n_seg + 1, dtype=torch.int32)
    seg_ptr[1:] = cnt.cumsum(0)
    T = int(cnt.sum())
    term_o = torch.randint(0, n, (T,), generator=g).int()
    term_w = torch.rand(T, generator=g)
    kind = torch.randint(0, 2, (T,), generator=g).int()
    zr = z.double().requires_grad_(True)
    seg_of = torch.repeat_interleave(torch.arange(n_seg), cnt)
    sq = ((zr[rows[seg_of]] - o.double()[term_o.long()]) ** 2).sum(1)
    want_s = [float(sq.detach()[kind == 0].sum()), float(sq.detach()[kind == 1].sum())]
    (sq * term_w.double()).sum().backward()
    touched = rows[cnt > 0]
    dev = [x.cuda() for x in (seg_ptr, rows.int(), term_o, term_w, kind)]
    zc, oc = z.cuda(), o.cuda()
    ws = torch.empty(L.gd_rowpair_mse_workspace(n_seg), device='cuda')

    def call(P):
        zv, ov = P.inp(zc), P.inp(oc)
        dz = P.out(n_seg if compact else n, d)
        sums = torch.zeros(2, device='cuda')
        _ok(L.gd_rowpair_mse_f32(_p(zv), zv.stride(0), _p(ov), ov.stride(0), d, _p(dev[0]), _p(dev[1]), n_seg, _p(dev[2]), _p(dev[3]), _p(dev[4]),
                                 _p(dz), dz.stride(0), compact, _p(sums), _p(ws), _st()), 'gd_rowpair_mse_f32')
        for k in range(2):                                 # (test_rowpair_mse_value_and_gradient's bound)
            assert abs(float(sums[k]) - want_s[k]) < 1e-4 * max(1, want_s[k])
        got = dz[(cnt > 0).cuda()] if compact else dz[touched.cuda()]
        _close(got, zr.grad[touched])
        if not compact:
            _assert_rows_untouched(dz, rows.cuda())
        return dict(sums=sums, dz=got)
    _all_layouts(call)


def test_rowtarget_mse_pair_pitched():
    """Two jobs in one launch (128-wide: loss sums only; 64-wide: gradient rows): ld_z_a, ld_z_b, ld_dz_b."""
    L = _L()
    g = torch.Generator(device='cuda').manual_seed(3)
    n = 9000
    assert L.gd_rowtarget_mse_pair_covers(128, 64) == 1
    jobs = []
    for d, rows in ((128, 7001), (64, 6500)):
        z = torch.randn(n, d, generator=g, device='cuda')
        ridx = torch.randperm(n, generator=g, device='cuda')[:rows].int()
        tm = torch.randn(rows, d, generator=g, device='cuda')
        coef = torch.rand(rows, generator=g, device='cuda')
        cnt = torch.randint(1, 5, (rows,), generator=g, device='cuda').float()
        kind = (torch.rand(rows, generator=g, device='cuda') < 0.3).int()
        df = z.double()[ridx.long()] - tm.double()
        sq = (df * df).sum(1) * cnt.double()
        jobs.append(dict(z=z, ridx=ridx, tm=tm, coef=coef, cnt=cnt, kind=kind, rows=rows, d=d, dz=coef.double()[:, None] * df,
                         sums=[sq[kind == 0].sum(), sq[kind == 1].sum()]))
    a, b = jobs

    def call(P):
        za, zb = P.inp(a['z']), P.inp(b['z'])
        dzb = P.out(n, 64)
        pa = torch.full((2 * L.gd_rowtarget_mse_blocks(a['rows']),), 5.0, device='cuda')
        pb = torch.full((2 * L.gd_rowtarget_mse_blocks(b['rows']),), 5.0, device='cuda')
        _ok(L.gd_rowtarget_mse_pair_f32(_p(za), za.stride(0), _p(a['tm']), 128, _p(a['ridx']), _p(a['coef']), _p(a['cnt']), _p(a['kind']), a['rows'],
                                        None, 0, _p(pa), _p(zb), zb.stride(0), _p(b['tm']), 64, _p(b['ridx']), _p(b['coef']), _p(b['cnt']),
                                        _p(b['kind']), b['rows'], _p(dzb), dzb.stride(0), _p(pb), _st()), 'gd_rowtarget_mse_pair_f32')
        for part, job in ((pa, a), (pb, b)):
            np.testing.assert_allclose(part.view(-1, 2).double().sum(0).cpu().numpy(), [float(v) for v in job['sums']], rtol=1e-5)
        _close(dzb[b['ridx'].long()], b['dz'])
        _assert_rows_untouched(dzb, b['ridx'])
        return dict(pa=pa, pb=pb, dz=dzb[b['ridx'].long()])
    _all_layouts(call)


@pytest.mark.parametrize('d', [64, 128, 16, 12])
@pytest.mark.parametrize('distmult', [False, True])
def test_edge_dot_bwd_pitched(d, distmult):
    """gd_edge_dot_bwd_f32 over a node-major incidence list (ld_z, ld_rel, ld_dz): repeated edges, self pairs, a hub of 320+
    incidences (the whole-wave path), isolated nodes (rows written as zeros)."""
    L = _L()
    g = torch.Generator().manual_seed(d + 1)
    n, m, r = 90, 700, 5
    z = torch.randn(n, d, generator=g)
    e = torch.randint(0, n - 7, (2, m), generator=g)
    e[:, :20] = e[:, 20:40]
    e[1, 40:50] = e[0, 40:50]
    e[0, 100:420] = 3
    rel = torch.randn(r, d, generator=g)
    et = torch.randint(0, r, (m,), generator=g)
    up = torch.randn(m, generator=g)
    zd = z.double().requires_grad_(True)
    ((zd[e[0]] * (rel.double()[et] if distmult else 1.0) * zd[e[1]]).sum(-1) * up.double()).sum().backward()
    ends_sorted, order = torch.sort(torch.cat([e[0], e[1]]), stable=True)
    edge = order % m
    other = torch.where(order >= m, e[0][edge], e[1][edge]).int().cuda()
    inc_ptr = torch.searchsorted(ends_sorted, torch.arange(n + 1)).cuda()
    w_inc, et_inc = up[edge].cuda(), et[edge].int().cuda()
    zc, rc_ = z.cuda(), rel.cuda()

    def call(P):
        zv = P.inp(zc)
        rv = P.inp(rc_) if distmult else None
        dz = P.out(n, d)
        _ok(L.gd_edge_dot_bwd_f32(_p(zv), zv.stride(0), d, _p(other), _p(w_inc), _p(rv), rv.stride(0) if distmult else 0,
                                  _p(et_inc) if distmult else None, _p(inc_ptr), n, _p(dz), dz.stride(0), _st()), 'gd_edge_dot_bwd_f32')
        _close(dz, zd.grad)
        assert float(dz[n - 7:].abs().max()) == 0.0
        return dict(dz=dz)
    _all_layouts(call)


@pytest.mark.parametrize('n,s,d', [(400, 300, 64), (90, 90, 128), (60, 45, 20), (50, 33, 32)])
def test_pairs_sigmoid_mse_pitched(n, s, d):
    """ld_z and ld_t (dz is compact by contract: the entry takes no pitch for it)."""
    L = _L()
    g = torch.Generator().manual_seed(n + s + d)
    z = torch.randn(n, d, generator=g) * 0.4
    nodes = torch.randperm(n, generator=g)[:s].sort().values
    s_pad = (s + 3) // 4 * 4
    target = torch.full((s, s_pad), -1.0)
    tri = torch.tril(torch.ones(s, s, dtype=torch.bool), -1) & (torch.rand(s, s, generator=g) < 0.9)      # 10 % of the pairs excluded
    target[:, :s][tri] = torch.rand(int(tri.sum()), generator=g)
    count = int(tri.sum())
    ii, jj = tri.nonzero(as_tuple=True)
    zd = z.double().requires_grad_(True)
    zs = zd[nodes]
    want = ((zs[ii] * zs[jj]).sum(-1).sigmoid() - target.double()[ii, jj]).pow(2).sum() / count
    want.backward()
    want = want.detach()
    zc, tc, nc = z.cuda(), target.cuda(), nodes.int().cuda()
    ws = torch.empty(L.gd_pairs_sigmoid_mse_workspace(s, d), device='cuda')

    def call(P):
        zv, tv = P.inp(zc), P.inp(tc)
        loss = torch.zeros((), device='cuda')
        dz = torch.full((s, d), SENTINEL, device='cuda')
        _ok(L.gd_pairs_sigmoid_mse_f32(_p(zv), zv.stride(0), _p(nc), s, d, _p(tv), tv.stride(0), 1.0 / count, _p(loss), _p(dz), _p(ws), _st()),
            'gd_pairs_sigmoid_mse_f32')
        assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want))
        _close(dz, zd.grad[nodes])
        return dict(loss=loss, dz=dz)
    _all_layouts(call)


# ------------------------------------------------------------------------------------------------ GAT (balanced forms)

@functools.lru_cache(maxsize=1)
def _gat_graph():
    """Hub rows in both directions (in-degree 1,500 / 300 / 70, out-degree alike): pieces + fix-up in the forward, group items
    in the one-launch backward and in the source-major aggregation."""
    from gnndelete_amd.graph import build_csr
    n = 6000
    g = torch.Generator().manual_seed(9)
    hubs = [(5, 1500), (77, 300), (5990, 70)]
    star_in = [torch.stack([torch.randperm(n, generator=g)[:k], torch.full((k,), h)]) for h, k in hubs]
    star_out = [torch.stack([torch.full((k,), h + 1), torch.randperm(n, generator=g)[:k]]) for h, k in hubs]
    ei = torch.cat([torch.randint(0, n, (2, 4 * n), generator=g)] + star_in + star_out, 1)
    ei = ei[:, ei[0] != ei[1]]
    key = torch.unique(ei[0] * n + ei[1])
    gr = build_csr(torch.stack([key // n, key % n]).cuda(), n, 'gat')
    assert gr.plan.n_split >= 2 and gr.plan_t.n_split >= 2
    return n, gr


def _gat_fp64(gr, n, h, a_src, a_dst, bias, dy, slope=0.2):
    """GATConv's aggregation over the CSR (self loops included) in fp64 + autograd: y, dh (message path), da_src, da_dst."""
    rows = torch.repeat_interleave(torch.arange(n, device='cuda'), (gr.rowptr[1:] - gr.rowptr[:-1]).long())
    col = gr.col.long()
    hd, s64, d64 = (t.double().requires_grad_(True) for t in (h, a_src, a_dst))
    e = torch.nn.functional.leaky_relu(s64[col] + d64[rows], slope)
    mx = torch.full((n,), -float('inf'), dtype=torch.float64, device='cuda').scatter_reduce(0, rows, e.detach(), 'amax')
    ex = (e - mx[rows]).exp()
    den = torch.zeros(n, dtype=torch.float64, device='cuda').index_add(0, rows, ex)
    alpha = ex / (den[rows] + 1e-16)
    y = torch.zeros(n, h.shape[1], dtype=torch.float64, device='cuda').index_add(0, rows, alpha[:, None] * hd[col]) + bias.double()
    y.backward(dy.double())
    return y.detach(), hd.grad, s64.grad, d64.grad


@pytest.mark.parametrize('h_rows_given', [True, False])
@pytest.mark.parametrize('d', [128, 64, 16])
def test_gat_aggregate_balanced_pitched(d, h_rows_given):
    """gd_gat_aggregate_balanced_f32: ldh, ldy; h_rows = the row count (32-bit row offsets) and 0 (64-bit addressing) give
    the same bits as each other, too."""
    L = _L()
    n, gr = _gat_graph()
    g = torch.Generator(device='cuda').manual_seed(d)
    r = lambda *s: torch.randn(*s, generator=g, device='cuda')
    h, a_src, a_dst, bias, dy = r(n, d), r(n), r(n), r(d), r(n, d)
    want = _gat_fp64(gr, n, h, a_src, a_dst, bias, dy)[0]
    plan = gr.plan
    scratch = plan.scratch_flat('gat', L.gd_gat_balanced_scratch(plan.n_slots, d), h.device)

    def run(P, h_rows):
        hv = P.inp(h)
        y = P.out(n, d)
        rowmax, rowsum = torch.full((n,), SENTINEL, device='cuda'), torch.full((n,), SENTINEL, device='cuda')
        _ok(L.gd_gat_aggregate_balanced_f32(_p(plan.items), plan.n_items, _p(plan.split), plan.n_split, plan.n_slots, _p(gr.col), _p(a_src), _p(a_dst),
                                            _p(hv), hv.stride(0), _p(y), y.stride(0), _p(bias), _p(rowmax), _p(rowsum), _p(scratch), 0.2, d,
                                            gr.nnz, h_rows, _st()), 'gd_gat_aggregate_balanced_f32')
        _close(y, want)
        return dict(y=y, rowmax=rowmax, rowsum=rowsum)
    _all_layouts(lambda P: run(P, n if h_rows_given else 0))
    a, b = run(_Pitched(1), n), run(_Pitched(1), 0)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize('pieces', ['0', '1'])
@pytest.mark.parametrize('d', [128, 64, 16])
def test_gat_backward_balanced_pitched(d, pieces, monkeypatch):
    """gd_gat_edge_grads_balanced_f32 (ldh, lddy; one-launch items, and GD_GAT_PIECES=1: the piece form) followed by the
    source-major aggregation: at d = 64 / 128 gd_spmm_csr_onepass_aux_f32 (x = dy at ldx, y = dh at ldy), at d = 16
    gd_gat_transpose_edges_f32 + the one-launch SpMM with edge values.  Bound: the 5e-5 of the GAT gradients in
    test_kernels_gpu.py."""
    from gnndelete_amd import ops
    monkeypatch.setenv('GD_GAT_PIECES', pieces)
    n, gr = _gat_graph()
    g = torch.Generator(device='cuda').manual_seed(d + 1)
    r = lambda *s: torch.randn(*s, generator=g, device='cuda')
    h, a_src, a_dst, bias, dy = r(n, d), r(n), r(n), r(d), r(n, d)
    _, dh_w, das_w, dad_w = _gat_fp64(gr, n, h, a_src, a_dst, bias, dy)
    _, rowmax, rowsum = ops.gat_forward_raw(gr, h, a_src, a_dst, bias, 0.2)

    def call(P):
        hv, dyv = P.inp(h), P.inp(dy)
        dh = P.out(n, d)
        got = ops.gat_backward_raw(gr, hv, a_src, a_dst, rowmax, rowsum, dyv, 0.2, bufs={'dh': dh})
        assert got[0].data_ptr() == dh.data_ptr()
        _close(dh, dh_w, 5e-5)
        _close(got[1], das_w, 5e-5)
        _close(got[2], dad_w, 5e-5)
        return dict(dh=dh, da_src=got[1].clone(), da_dst=got[2].clone())
    _all_layouts(call)


# ------------------------------------------------------------------------------------------------ typed conv (R-GCN)

@functools.lru_cache(maxsize=1)
def _typed_graph():
    from gnndelete_amd.graph import TypedNodeCSR
    n, m, R = 300, 6000, 30
    g = torch.Generator().manual_seed(21)
    ei = torch.randint(0, n - 3, (2, m), generator=g)
    et = torch.randint(0, R - 1, (m,), generator=g)
    return n, R, ei, et, TypedNodeCSR(ei.cuda(), et.cuda(), n, R)


@pytest.mark.parametrize('trans', [0, 1])
@pytest.mark.parametrize('form,din,dout,nb', [('wave', 128, 64, 4), ('wave', 64, 64, 4), ('tile', 128, 64, 4), ('tile', 128, 128, 4),
                                              ('node', 128, 64, 4), ('node', 24, 12, None)])
def test_typed_conv_pitched(form, din, dout, nb, trans, monkeypatch):
    """gd_rgcn_wave_conv_f32, gd_rgcn_tile_conv_f32, gd_rgcn_conv_f32: x at ldx, y (which holds the root term on entry and is
    accumulated into) at ldy; forward and the transposed direction, against the fp64 restatement of RGCNConv."""
    from gnndelete_amd import ops
    from oracle import pyg_semantics as pyg
    if form == 'tile':
        monkeypatch.setenv('GD_RGCN_WAVE', '0')
    if form == 'node':
        monkeypatch.setenv('GD_RGCN_NODE_MAJOR', '1')
    n, R, ei, et, tg = _typed_graph()
    n_blocks = 1 if nb is None else nb
    if form != 'node':                                   # (the node-major switch is read by the dispatcher, not by this query)
        assert ops.rgcn_wave_form(*((dout, din) if trans else (din, dout)), n_blocks, n, 2 * max(din, dout)) == (form == 'wave')
    g = torch.Generator().manual_seed(din + dout)
    x = torch.randn(n, din, generator=g, dtype=torch.float64)
    w = torch.randn((R, din, dout) if nb is None else (R, nb, din // nb, dout // nb), generator=g, dtype=torch.float64) * 0.2
    up = torch.randn(n, dout, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    y64 = pyg.rgcn_conv(xr, ei, et, w, torch.zeros(din, dout, dtype=torch.float64), torch.zeros(dout, dtype=torch.float64), nb)
    y64.backward(up)
    src64, want = (up, xr.grad) if trans else (x, y64.detach())
    base = torch.randn(n, din if trans else dout, generator=g)
    src, wg, bg = src64.float().cuda(), w.float().cuda(), base.cuda()

    def call(P):
        xv = P.inp(src)
        y = P.out(n, bg.shape[1], init=bg)
        ops.rgcn_typed_accumulate(tg, xv, wg, n_blocks, trans, y)
        _close(y, base.double() + want)
        return dict(y=y)
    _all_layouts(call)


@pytest.mark.parametrize('din,dout,nb', [(128, 64, 4), (128, 128, 4), (24, 12, 1), (32, 32, 4)])
def test_typed_wgrad_and_edge_dot_pitched(din, dout, nb):
    """gd_typed_wgrad_f32 and gd_typed_edge_dot_f32 (the trainable relation weights' gradients): x at ldx, dy at ldy."""
    L = _L()
    n, R, ei, et, _ = _typed_graph()
    g = torch.Generator().manual_seed(din + 3 * dout)
    order = torch.argsort(et, stable=True)
    src, dst, rel = ei[0][order], ei[1][order], et[order]
    rel_ptr = torch.zeros(R + 1, dtype=torch.int32)
    rel_ptr[1:] = torch.bincount(rel, minlength=R).cumsum(0)
    m = src.numel()
    ew = torch.rand(m, generator=g)
    x, dy = torch.randn(n, din, generator=g), torch.randn(n, dout, generator=g)
    w = torch.randn(R, nb, din // nb, dout // nb, generator=g) * 0.2
    xb = x.double()[src].view(m, nb, din // nb)
    db = dy.double()[dst].view(m, nb, dout // nb)
    dw_want = torch.zeros(R, nb, din // nb, dout // nb, dtype=torch.float64).index_add_(
        0, rel, ew.double()[:, None, None, None] * xb[:, :, :, None] * db[:, :, None, :])
    dot_want = torch.einsum('ebi,ebio,ebo->e', xb, w.double()[rel], db)
    dev = [t.cuda() for t in (rel_ptr, src.int(), dst.int(), rel.int(), ew, x, dy, w)]

    def call(P):
        xv, dyv = P.inp(dev[5]), P.inp(dev[6])
        dw = torch.full_like(dev[7], SENTINEL)
        out = torch.full((m,), SENTINEL, device='cuda')
        _ok(L.gd_typed_wgrad_f32(_p(dev[0]), R, _p(dev[1]), _p(dev[2]), _p(dev[4]), _p(xv), xv.stride(0), _p(dyv), dyv.stride(0), nb, din, dout,
                                 _p(dw), _st()), 'gd_typed_wgrad_f32')
        _ok(L.gd_typed_edge_dot_f32(_p(dev[1]), _p(dev[2]), _p(dev[3]), m, _p(xv), xv.stride(0), _p(dyv), dyv.stride(0), _p(dev[7]), nb, din, dout,
                                    _p(out), _st()), 'gd_typed_edge_dot_f32')
        _close(dw, dw_want)
        _close(out, dot_want)
        return dict(dw=dw, out=out)
    _all_layouts(call)
