"""The kernels of the step with conv1's weight folded into W_D1, called directly: gd_del1_chain_fold_loss_wgrad_f32 (the chained Del-1
pass on a = A^ x with W1^T W_D1 and the bias row b1 W_D1), gd_step_tail_fold1_f32 (dW_D1 = W1 G + b1^T s per column, Adam, the next
step's fold) and gd_layer1_fold_f32 (the fold from scratch).

Row counts: 65,536 (the smallest the form covers) and 65,541 (a last 16-row unit of five live rows, eleven clamped duplicates);
scattered rows of an 80,000-row table; one case with row pitches wider than the widths (a 136, z 144, dt 72).  Non-zero folded bias,
non-zero dt, a random previous sign pattern, a ninth of the rows without a loss slot.  W_D = I + 0.05 randn is not symmetric and W1 is
a dense random matrix, so a transposed operand anywhere shows.

Bounds.  TOL = 1e-5 is the bound tests/test_kernels_gpu.py puts on one fp32 product or sum against fp64.  A value that went through
k chained fp32 stages, each a 128-term product or a sum over the rows, is held to k * TOL (errors of successive stages add to first
order):
  the pass alone, against fp64 of the FOLDED formulas on the same fp32 inputs (w_fold given): z, loss sums, G, s - one stage, TOL;
  the tail alone, against fp64 of its formulas on the same partials: dW (reduction, then W1 G: 2 TOL), Adam state (2 TOL), the next
    fold (a third product: 3 TOL);
  the composition against fp64 of the UNFOLDED formulas on pre1 = a W1^T + b1: fold (1) -> z (2) -> G, s (3: sums over the rows of
    values that carry z's error) -> W1 G (4): 4 TOL for dW_D1 and the Adam state, 5 TOL for the next fold.  The unfolded kernels on
    the fp32 pre1 are held to the same 4 TOL (pre1 is a rounded 128-term product as well), so the two forms meet one bar.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5                                   # tests/test_kernels_gpu.py
N, D, O = 80000, 128, 64
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _lib():
    from gnndelete_amd import _lib
    return _lib.lib()


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, what):
    from gnndelete_amd._lib import check
    check(rc, what)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _pitched(t, pitch):
    """A [rows, pitch] NaN buffer whose first columns hold t; returns the [rows, width] view."""
    buf = torch.full((t.shape[0], pitch), float('nan'), device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


@functools.lru_cache(maxsize=None)
def _data(n_sel):
    """The input of one row count, built once and never modified.  The index list carries 16 entries BEHIND n_sel that name rows of
    NaNs: a pass that read past the end instead of clamping would show them."""
    g = torch.Generator(device='cuda').manual_seed(2000 + n_sel)
    dev = 'cuda'

    def randn(*shape):
        return torch.randn(*shape, device=dev, generator=g)
    a = randn(N, D)
    w1 = (randn(D, D) / D ** 0.5).contiguous()
    b1 = (0.5 * randn(D)).contiguous()
    wd = (torch.eye(D, device=dev) + 0.05 * randn(D, D)).contiguous()
    perm = torch.randperm(N, device=dev, generator=g)
    idx = torch.sort(perm[:n_sel]).values.to(torch.int32)
    bad = perm[n_sel:n_sel + 16]
    a[bad] = float('nan')
    idx_buf = torch.cat([idx, bad.to(torch.int32)]).contiguous()
    n_slots = n_sel - n_sel // 9
    slot = torch.full((n_sel + 16,), -1, dtype=torch.int32, device=dev)
    slot[torch.randperm(n_sel, device=dev, generator=g)[:n_slots]] = torch.randperm(n_slots, device=dev, generator=g).to(torch.int32)
    if int(slot[n_sel - 1]) < 0:                                  # the last row carries a loss term (the duplicates test scales it up)
        j = int((slot[:n_sel] >= 0).nonzero()[0])
        slot[n_sel - 1], slot[j] = slot[j].clone(), -1
    tm = randn(n_slots, D)
    coef = torch.rand(n_slots, device=dev, generator=g) * 1e-3
    cnt = torch.randint(1, 4, (n_slots,), device=dev, generator=g).float() * torch.where(torch.rand(n_slots, device=dev, generator=g) < 0.3, -1.0, 1.0)
    dt = 1e-3 * randn(N, O)
    w_next = (randn(O, D) / 8).contiguous()
    prev = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_sel + 16, 4), device=dev, dtype=torch.int64, generator=g).to(torch.int32)
    wf = (w1.double().t() @ wd.double()).float().contiguous()
    bf = (b1.double() @ wd.double()).float().contiguous()
    assert float(bf.abs().min()) > 0
    return dict(a=a, w1=w1, b1=b1, wd=wd, idx=idx_buf, slot=slot, tm=tm, coef=coef, cnt=cnt, dt=dt, w_next=w_next, prev=prev, wf=wf, bf=bf,
                s=n_sel)


def _fold_pass(Dt, a, pitched=False):
    """(z [N, D] view, sign words, loss partials, transposed partial matrices [nb, c, i], column-sum partials [nb, D], nb)."""
    L, s = _lib(), Dt['s']
    nb = L.gd_del1_loss_wgrad_parts(s)
    assert L.gd_del1_chain_fold_covers(s, D, D) == 1 and 1 <= nb <= L.gd_rows_gemm_wgrad_blocks(s)
    dt = Dt['dt']
    z = torch.full((N, D), float('nan'), device='cuda')
    if pitched:
        a, dt, z = _pitched(a, 136), _pitched(dt, 72), _pitched(z, 144)
    bits = Dt['prev'].clone()
    lp = torch.full((2 * nb,), 5.0, device='cuda')
    ws = torch.full((max(nb * D * D, L.gd_rows_gemm_wgrad_workspace(s, D, D)),), 3.0, device='cuda')
    cs = torch.full((nb * D,), 7.0, device='cuda')
    _ok(L.gd_del1_chain_fold_loss_wgrad_f32(_p(a), a.stride(0), _p(Dt['idx']), s, _p(Dt['wf']), _p(Dt['bf']), D, _p(z), z.stride(0), _p(bits),
                                            _p(Dt['slot']), _p(Dt['tm']), _p(Dt['coef']), _p(Dt['cnt']), _p(dt), dt.stride(0), O, _p(Dt['w_next']),
                                            _p(lp), _p(ws), _p(cs), nb, _st()), 'fold pass')
    torch.cuda.synchronize()
    return z, bits, lp, ws[:nb * D * D].view(nb, D, D), cs.view(nb, D), nb


def _gate(prev, s):
    return ((prev[:s].long()[:, :, None] >> torch.arange(32, device='cuda')) & 1).reshape(s, D).bool()


def _g64(Dt, z64, s):
    """fp64 gradient rows of the pass from its z: coef (z - tm) on the rows with a loss slot + the gated previous gradient."""
    li = Dt['idx'][:s].long()
    slot = Dt['slot'][:s]
    has, u = slot >= 0, slot.clamp(min=0).long()
    diff = z64 - Dt['tm'].double()[u]
    dh = Dt['dt'].double()[li] @ Dt['w_next'].double()
    g = torch.where(has[:, None], Dt['coef'].double()[u][:, None] * diff, torch.zeros_like(z64)) + torch.where(_gate(Dt['prev'], s), dh, torch.zeros_like(dh))
    sq = (diff * diff).sum(1) * has
    cn = Dt['cnt'].double()[u]
    return g, float((sq * cn.clamp(min=0)).sum()), float((sq * (-cn).clamp(min=0)).sum())


def test_coverage_query_and_refusals():
    L = _lib()
    assert L.gd_del1_chain_fold_covers(65536, 128, 128) == 1
    for n_sel, d, h in ((65535, 128, 128), (65536, 64, 128), (65536, 128, 64), (65536, 256, 128), (65536, 64, 64), (0, 128, 128)):
        assert L.gd_del1_chain_fold_covers(n_sel, d, h) == 0, (n_sel, d, h)
    # the fold tail has no accumulating form
    t = torch.zeros(128 * 128, device='cuda')
    i32 = torch.zeros(4, dtype=torch.int32, device='cuda')
    args = lambda acc1, d1: (_p(t), _p(t), 1, d1, acc1, _p(t), _p(t), _p(t.clone()), _p(t.clone()), _p(t.clone()), _p(t.clone()), _p(t.clone()),
                             _p(t.clone()), _p(t), 1, 64, 0, _p(t.clone()), _p(t.clone()), _p(t.clone()), _p(t.clone()), LR, B1, B2, EPS, _p(t), 1,
                             _p(t), 1, _p(t.clone()), 4, _p(i32), _p(i32[1:]), _p(i32[2:]), _st())
    from gnndelete_amd._lib import GnnDeleteHipError
    for acc1, d1 in ((1, 128), (0, 64)):
        with pytest.raises(GnnDeleteHipError):
            _ok(L.gd_step_tail_fold1_f32(*args(acc1, d1)), 'refused')
    torch.cuda.synchronize()


@pytest.mark.parametrize('n_sel,pitched', [(65536, False), (65541, False), (65541, True)])
def test_fold_pass_against_fp64(n_sel, pitched):
    Dt = _data(n_sel)
    s = Dt['s']
    z, bits, lp, wst, cs, nb = _fold_pass(Dt, Dt['a'], pitched)
    li = Dt['idx'][:s].long()
    z64 = Dt['a'].double()[li] @ Dt['wf'].double() + Dt['bf'].double()
    g64, ls0, ls1 = _g64(Dt, z64, s)
    G64, s64 = Dt['a'].double()[li].t() @ g64, g64.sum(0)
    G = wst.double().sum(0).t()                                   # [c][i] partials -> G[i][c]
    errs = dict(z=_rel(z[li], z64), G=_rel(G, G64), s=_rel(cs.double().sum(0), s64),
                loss_dec=abs(float(lp[0::2].double().sum()) - ls0) / ls0, loss_ni=abs(float(lp[1::2].double().sum()) - ls1) / ls1)
    no_bias = _rel((Dt['a'].double()[li] @ Dt['wf'].double()), z64)
    print(f'[fold pass n_sel={n_sel} pitched={pitched}] MEASURED rel. error to fp64: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items())
          + f'; without the bias row z would be {no_bias:.2e} off; G^T instead of G {_rel(G.t(), G64):.2e}')
    assert no_bias > 1e3 * TOL and _rel(G.t(), G64) > 1e3 * TOL
    for k, v in errs.items():
        assert v <= TOL, (k, v)
    # sign bits: the pattern of the kernel's OWN z (a folded z may land on the other side of zero from an unfolded one)
    own = (z[li] > 0)
    got = _gate(bits, s)
    assert torch.equal(got, own)
    assert torch.equal(bits[s:], Dt['prev'][s:])                  # nothing written behind the rows
    # rows outside the list (and the padding columns) untouched
    listed = torch.zeros(N, dtype=torch.bool, device='cuda')
    listed[li] = True
    assert bool(torch.isnan(z[~listed]).all()) and not bool(torch.isnan(z[listed]).any())
    if pitched:
        assert bool(torch.isnan(z.as_strided((N, 144 - D), (144, 1), D)).all())
    assert not bool(torch.isnan(wst).any()) and not bool(torch.isnan(cs).any()) and not bool(torch.isnan(lp).any())


def test_column_sums_skip_the_clamped_duplicates_of_the_last_row():
    """The last 16-row unit of 65,541 rows holds eleven duplicates of the last row.  With that row 100,000 times larger than the rest it
    dominates s; counted twelve times instead of once, s would be an order of magnitude off."""
    Dt = _data(65541)
    s = Dt['s']
    li = Dt['idx'][:s].long()
    a = Dt['a'].clone()
    a[li[-1]] *= 1e5
    _, _, _, wst, cs, _ = _fold_pass(Dt, a)
    z64 = a.double()[li] @ Dt['wf'].double() + Dt['bf'].double()
    g64, _, _ = _g64(Dt, z64, s)
    assert int(Dt['slot'][s - 1]) >= 0, 'the last row needs a loss term for its g to be large'
    s64 = g64.sum(0)
    counted = s64 + 11 * g64[-1]
    err = _rel(cs.double().sum(0), s64)
    print(f'[fold pass duplicates] MEASURED s rel. error {err:.2e}; with the duplicates counted it would be {_rel(counted, s64):.2e}; '
          f'the last row is {float(g64[-1].norm() / s64.norm()):.2f} of s')
    assert _rel(counted, s64) > 1.0
    assert err <= TOL
    assert _rel(wst.double().sum(0).t(), a.double()[li].t() @ g64) <= TOL


def _adam64(p, m, v, g, t):
    m = m + (g - m) * (1 - B1)
    v = B2 * v + (1 - B2) * g * g
    den = v.sqrt() / (1 - B2 ** t) ** 0.5 + EPS
    return p - (LR / (1 - B1 ** t)) * m / den, m, v


def _tail_state(gen, it):
    r = lambda *sh: torch.randn(*sh, device='cuda', generator=gen)
    return dict(wd2=(torch.eye(O, device='cuda') + 0.05 * r(O, O)).contiguous(), m1=1e-3 * r(D, D), v1=1e-6 * r(D, D).abs(), m2=1e-3 * r(O, O),
                v2=1e-6 * r(O, O).abs(), parts2=r(3, O, O), lp1=r(2 * 5).abs(), lp2=r(2 * 7).abs(), hist=torch.zeros(8, 4, device='cuda'),
                pos=torch.full((1,), 2, dtype=torch.int32, device='cuda'), iter=torch.full((1,), it, dtype=torch.int32, device='cuda'),
                arrive=torch.zeros(2, dtype=torch.int32, device='cuda'))


def _run_fold_tail(parts_t, cs, w1, b1, wd, st):
    """-> dict of everything gd_step_tail_fold1_f32 writes (inputs are cloned)."""
    L = _lib()
    o = {k: v.clone() for k, v in st.items()}
    o.update(wd=wd.clone(), g1=torch.full((D, D), float('nan'), device='cuda'), g2=torch.full((O, O), float('nan'), device='cuda'),
             wf=torch.full((D, D), float('nan'), device='cuda'), bf=torch.full((D,), float('nan'), device='cuda'))
    _ok(L.gd_step_tail_fold1_f32(_p(parts_t), _p(cs), parts_t.shape[0], D, 0, _p(w1), _p(b1), _p(o['g1']), _p(o['wd']), _p(o['m1']), _p(o['v1']),
                                 _p(o['wf']), _p(o['bf']), _p(o['parts2']), o['parts2'].shape[0], O, 0, _p(o['g2']), _p(o['wd2']), _p(o['m2']),
                                 _p(o['v2']), LR, B1, B2, EPS, _p(o['lp1']), 5, _p(o['lp2']), 7, _p(o['hist']), 8, _p(o['pos']), _p(o['iter']),
                                 _p(o['arrive']), _st()), 'fold tail')
    torch.cuda.synchronize()
    return o


def _run_parts_tail(parts, wd, st):
    L = _lib()
    o = {k: v.clone() for k, v in st.items()}
    o.update(wd=wd.clone(), g1=torch.full((D, D), float('nan'), device='cuda'), g2=torch.full((O, O), float('nan'), device='cuda'))
    _ok(L.gd_step_tail_parts_f32(_p(parts), parts.shape[0], D, 0, _p(o['g1']), _p(o['wd']), _p(o['m1']), _p(o['v1']), _p(o['parts2']),
                                 o['parts2'].shape[0], O, 0, _p(o['g2']), _p(o['wd2']), _p(o['m2']), _p(o['v2']), LR, B1, B2, EPS, _p(o['lp1']), 5,
                                 _p(o['lp2']), 7, _p(o['hist']), 8, _p(o['pos']), _p(o['iter']), _p(o['arrive']), _st()), 'parts tail')
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize('n_part', [1, 256])
def test_fold_tail_alone(n_part):
    gen = torch.Generator(device='cuda').manual_seed(77 + n_part)
    Dt = _data(65536)
    w1, b1, wd = Dt['w1'], Dt['b1'], Dt['wd']
    parts_t = torch.randn(n_part, D, D, device='cuda', generator=gen)
    cs = torch.randn(n_part, D, device='cuda', generator=gen)
    it = 4
    st = _tail_state(gen, it)
    o = _run_fold_tail(parts_t, cs, w1, b1, wd, st)
    G64, s64 = parts_t.double().sum(0).t(), cs.double().sum(0)
    dw64 = w1.double() @ G64 + b1.double()[:, None] * s64[None, :]
    wd64, m64, v64 = _adam64(wd.double(), st['m1'].double(), st['v1'].double(), dw64, it + 1)
    errs = dict(dW=_rel(o['g1'], dw64), W_D=_rel(o['wd'], wd64), m=_rel(o['m1'], m64), v=_rel(o['v1'], v64),
                Wf=_rel(o['wf'], w1.double().t() @ wd64), bf=_rel(o['bf'], b1.double() @ wd64))
    print(f'[fold tail n_part={n_part}] MEASURED rel-L2 to fp64: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items())
          + f'; the b1 s term is {float((b1.double()[:, None] * s64[None, :]).norm() / dw64.norm()):.2f} of dW; the update moved W_D by '
          f'{_rel(o["wd"], wd):.2e}; Wf from the OLD W_D would be {_rel(w1.double().t() @ wd.double(), w1.double().t() @ wd64):.2e} off')
    for k, v in errs.items():
        assert v <= (3 if k in ('Wf', 'bf') else 2) * TOL, (k, v)
    assert _rel(w1.double().t() @ wd.double(), w1.double().t() @ wd64) > 10 * 3 * TOL        # the fold is of the UPDATED weight
    # weight 2, the loss log and the counters: the bits of the unfolded tail on the same input
    ref = _run_parts_tail(parts_t, wd, st)
    for k in ('g2', 'wd2', 'm2', 'v2', 'hist', 'pos', 'iter', 'arrive'):
        assert torch.equal(o[k], ref[k]), k
    assert int(o['iter']) == it + 1 and int(o['pos']) == 3 and int(o['arrive'][0]) == 0
    # twice the same bits
    o2 = _run_fold_tail(parts_t, cs, w1, b1, wd, st)
    for k in ('g1', 'wd', 'm1', 'v1', 'wf', 'bf'):
        assert torch.equal(o[k], o2[k]), k


def test_construction_fold_against_fp64():
    L, Dt = _lib(), _data(65536)
    wf, bf = torch.full((D, D), float('nan'), device='cuda'), torch.full((D,), float('nan'), device='cuda')
    _ok(L.gd_layer1_fold_f32(_p(Dt['w1']), _p(Dt['b1']), _p(Dt['wd']), _p(wf), _p(bf), _st()), 'fold')
    torch.cuda.synchronize()
    want = Dt['w1'].double().t() @ Dt['wd'].double()
    e_w, e_b = _rel(wf, want), _rel(bf, Dt['b1'].double() @ Dt['wd'].double())
    print(f'[layer-1 fold] MEASURED rel-L2 to fp64: Wf {e_w:.2e}, bf {e_b:.2e}; W1 W_D instead of W1^T W_D would be '
          f'{_rel(Dt["w1"].double() @ Dt["wd"].double(), want):.2e}')
    assert e_w <= TOL and e_b <= TOL
    assert _rel(Dt['w1'].double() @ Dt['wd'].double(), want) > 1e3 * TOL
    # ... and it is what the fold tail leaves for an unchanged weight: a zero gradient with zero moments moves nothing
    gen = torch.Generator(device='cuda').manual_seed(3)
    st = _tail_state(gen, 0)
    st['m1'].zero_()
    st['v1'].zero_()
    o = _run_fold_tail(torch.zeros(2, D, D, device='cuda'), torch.zeros(2, D, device='cuda'), Dt['w1'], Dt['b1'], Dt['wd'], st)
    assert torch.equal(o['wd'], Dt['wd']) and torch.equal(o['wf'], wf) and torch.equal(o['bf'], bf)


def test_fold_composes_like_the_unfolded_pass_and_tail():
    """Folded pass + fold tail against gd_del1_chain_loss_wgrad_f32 + gd_step_tail_parts_f32 on pre1 = a W1^T + b1, both to fp64."""
    L = _lib()
    Dt = _data(65541)
    s = Dt['s']
    li = Dt['idx'][:s].long()
    gen = torch.Generator(device='cuda').manual_seed(11)
    it = 2
    st = _tail_state(gen, it)
    w1, b1, wd = Dt['w1'], Dt['b1'], Dt['wd']
    # fp64 of the unfolded formulas
    pre64 = Dt['a'].double()[li] @ w1.double().t() + b1.double()
    g64, _, _ = _g64(Dt, pre64 @ wd.double(), s)
    dw64 = pre64.t() @ g64
    wd64, m64, v64 = _adam64(wd.double(), st['m1'].double(), st['v1'].double(), dw64, it + 1)
    # folded
    z_f, _, _, wst, cs, nb = _fold_pass(Dt, Dt['a'])
    f = _run_fold_tail(wst.contiguous(), cs.contiguous(), w1, b1, wd, st)
    # unfolded, on the fp32 rounding of the fp64 pre1 (rows outside the list: zeros, never read)
    pre1 = torch.zeros(N, D, device='cuda')
    pre1[li] = pre64.float()
    z_u, bits = torch.zeros(N, D, device='cuda'), Dt['prev'].clone()
    lp, ws = torch.zeros(2 * nb, device='cuda'), torch.zeros(max(nb * D * D, L.gd_rows_gemm_wgrad_workspace(s, D, D)), device='cuda')
    _ok(L.gd_del1_chain_loss_wgrad_f32(_p(pre1), pre1.stride(0), _p(Dt['idx']), s, _p(wd), D, _p(z_u), z_u.stride(0), _p(bits), _p(Dt['slot']),
                                       _p(Dt['tm']), _p(Dt['coef']), _p(Dt['cnt']), _p(Dt['dt']), Dt['dt'].stride(0), O, _p(Dt['w_next']), None, None,
                                       None, None, _p(lp), _p(ws), nb, _st()), 'unfolded pass')
    u = _run_parts_tail(ws[:nb * D * D].view(nb, D, D).contiguous(), wd, st)
    want = dict(g1=dw64, wd=wd64, m1=m64, v1=v64)
    e_f = {k: _rel(f[k], w) for k, w in want.items()}
    e_u = {k: _rel(u[k], w) for k, w in want.items()}
    e_next = dict(wf=_rel(f['wf'], w1.double().t() @ wd64), bf=_rel(f['bf'], b1.double() @ wd64))
    print('[fold composition] MEASURED rel-L2 to fp64 (folded / unfolded): ' + ', '.join(f'{k} {e_f[k]:.2e} / {e_u[k]:.2e}' for k in want)
          + f'; next fold Wf {e_next["wf"]:.2e}, bf {e_next["bf"]:.2e}; z of the two forms {_rel(z_f[li], z_u[li]):.2e} apart; '
          f'the bias term b1^T s is {float((b1.double()[:, None] * g64.sum(0)[None, :]).norm() / dw64.norm()):.2e} of dW_D1')
    for k in want:
        assert e_f[k] <= 4 * TOL, (k, e_f[k])
        assert e_u[k] <= 4 * TOL, (k, e_u[k])
    assert e_next['wf'] <= 5 * TOL and e_next['bf'] <= 5 * TOL
    assert _rel(z_f[li], z_u[li]) <= 2 * TOL
