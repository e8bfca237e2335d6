"""The end-of-step launches against each other and against fp64: gd_step_tail_parts_f32 / gd_step_tail_f32 (both split-K
reductions with Adam + the loss finalize in ONE launch whose blocks meet through global memory) must leave the same BITS as
gd_rows_gemm_wgrad_reduce_f32 (+ Adam) twice followed by gd_loss_finalize_f32 - the kernel's documented contract - and both
must agree with the fp64 sums and with torch.optim.Adam.  Also the small entries nothing else calls directly
(gd_loss_finalize_f32 with extra_sums, gd_gate_rows_f32, gd_segment_sum_f32) and the refusals of the tail entries.

Every tail call here starts from `arrive` = 0 and a non-negative iteration counter, exactly as the engine does: the kernel
waits on `arrive`, so no case may hand it any other state."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import rel_l2

gpu = pytest.mark.gpu
TOL = 1e-5                                # tests/test_kernels_gpu.py's bound for every fp32 kernel against fp64
HYPER = (1e-2, 0.9, 0.999, 1e-8)
SENTINEL = -777.25                        # history rows nobody has written yet


def _L():
    from gnndelete_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(rc, what):
    from gnndelete_amd import _lib
    _lib.check(rc, what)


class _Case:
    """The inputs of K consecutive steps (fresh partial matrices and loss partials every step) and the initial state."""

    def __init__(self, d1, d2, np1, np2, acc1=0, acc2=0, n1=3, n2=5, capacity=4, K=3, t0=0, seed=0, rows=None):
        self.d = (d1, d2)
        self.np = (np1, np2)
        self.rows = rows                                  # (n_sel1, n_sel2) of the row-count form, else None
        self.acc = (acc1, acc2)
        self.n = (n1, n2)
        self.capacity, self.K, self.t0 = capacity, K, t0
        g = torch.Generator(device='cuda').manual_seed(1000 + seed)
        r = lambda *s: torch.randn(*s, generator=g, device='cuda')
        # partial matrices of different magnitudes, so that a dropped or doubled one shows in the fp64 comparison; every
        # element carries a fixed sign with a mean of three standard deviations, so that no reduced gradient entry sits within
        # rounding of zero (Adam's first step is lr g / (|g| + eps): the torch.optim comparison is ill-conditioned there)
        self.parts = []
        for n, d in zip(self.np, self.d):
            sign = torch.where(torch.rand(d, d, generator=g, device='cuda') < 0.5, -3.0, 3.0)
            scale = 1e-2 * 10.0 ** -(torch.arange(n, device='cuda') % 3).float()
            self.parts.append((r(K, n, d, d) + sign) * scale[None, :, None, None])
        self.lp = [torch.rand(K, max(n, 1), 2, generator=g, device='cuda') + 0.01 for n in self.n]
        self.p0 = [r(d, d) * 1e-1 for d in self.d]
        nontrivial = t0 > 0
        self.m0 = [r(d, d) * 1e-3 if nontrivial else torch.zeros(d, d, device='cuda') for d in self.d]
        self.v0 = [torch.rand(d, d, generator=g, device='cuda') * 1e-6 if nontrivial else torch.zeros(d, d, device='cuda')
                   for d in self.d]
        self.dw0 = [r(d, d) * 1e-2 for d in self.d]       # what `accumulate` adds to in the first step
        self.pos0 = 1 % capacity

    def separate_rows(self, k):
        """The row count the separate reduction entry is given for weight k: it takes rows, not partials."""
        if self.rows is not None:
            return self.rows[k]
        n_sel = 128 * self.np[k]
        assert self.np[k] <= 512
        return n_sel


class _State:
    def __init__(self, c):
        self.dw = [x.clone() for x in c.dw0]
        self.p = [x.clone() for x in c.p0]
        self.m = [x.clone() for x in c.m0]
        self.v = [x.clone() for x in c.v0]
        self.hist = torch.full((c.capacity, 4), SENTINEL, device='cuda')
        self.pos = torch.tensor([c.pos0], dtype=torch.int32, device='cuda')
        self.iter = torch.tensor([c.t0], dtype=torch.int32, device='cuda')
        self.arrive = torch.zeros(2, dtype=torch.int32, device='cuda')          # the engine's zero-initialised counter
        # the partials of the step in flight live in STATIC buffers (what a captured graph needs; the eager runs do the same)
        self.parts = [torch.empty_like(x[0]) for x in c.parts]
        self.lp = [torch.empty_like(x[0]) for x in c.lp]

    def load(self, c, step):
        for dst, src in zip(self.parts + self.lp, c.parts + c.lp):
            dst.copy_(src[step])

    def snapshot(self):
        """Device clones (stream-ordered: no host synchronisation between two launches)."""
        return [x.clone() for x in self.dw + self.p + self.m + self.v + [self.hist, self.pos, self.iter, self.arrive]]


NAMES = ['dw1', 'dw2', 'param1', 'param2', 'exp_avg1', 'exp_avg2', 'exp_avg_sq1', 'exp_avg_sq2', 'hist', 'pos', 'iter', 'arrive']


def _lp(c, s, k):
    """Loss partials of layer k; a count of 0 goes with a NULL pointer (the entries accept that: nothing is read)."""
    return s.lp[k].data_ptr() if c.n[k] else None


def _separate(c, s):
    L, st = _L(), _stream()
    for k in range(2):
        n_sel = c.separate_rows(k)
        assert L.gd_rows_gemm_wgrad_blocks(n_sel) == c.np[k], (n_sel, c.np[k])
        _check(L.gd_rows_gemm_wgrad_reduce_f32(s.parts[k].data_ptr(), n_sel, c.d[k], c.d[k], s.dw[k].data_ptr(), c.acc[k],
                                               s.p[k].data_ptr(), s.m[k].data_ptr(), s.v[k].data_ptr(), s.iter.data_ptr(), *HYPER, st),
               'gd_rows_gemm_wgrad_reduce_f32')
    _check(L.gd_loss_finalize_f32(_lp(c, s, 0), c.n[0], _lp(c, s, 1), c.n[1], None, s.hist.data_ptr(), c.capacity,
                                  s.pos.data_ptr(), s.iter.data_ptr(), st), 'gd_loss_finalize_f32')


def _tail(c, s, by_rows=False):
    L = _L()
    fn = L.gd_step_tail_f32 if by_rows else L.gd_step_tail_parts_f32
    cnt = c.rows if by_rows else c.np
    _check(fn(s.parts[0].data_ptr(), cnt[0], c.d[0], c.acc[0], s.dw[0].data_ptr(), s.p[0].data_ptr(), s.m[0].data_ptr(), s.v[0].data_ptr(),
              s.parts[1].data_ptr(), cnt[1], c.d[1], c.acc[1], s.dw[1].data_ptr(), s.p[1].data_ptr(), s.m[1].data_ptr(), s.v[1].data_ptr(),
              *HYPER, _lp(c, s, 0), c.n[0], _lp(c, s, 1), c.n[1], s.hist.data_ptr(), c.capacity, s.pos.data_ptr(),
              s.iter.data_ptr(), s.arrive.data_ptr(), _stream()), 'gd_step_tail')


def _run(c, launch):
    s = _State(c)
    snaps = []
    for step in range(c.K):
        s.load(c, step)
        launch(c, s)
        snaps.append(s.snapshot())
    torch.cuda.synchronize()
    return [[x.cpu() for x in snap] for snap in snaps]


def _assert_same_bits(a, b, what):
    for step, (sa, sb) in enumerate(zip(a, b)):
        for name, x, y in zip(NAMES, sa, sb):
            if name == 'arrive':
                continue                                   # (the separate launches never touch it)
            assert torch.equal(x, y), f'{what}: {name} differs after step {step + 1}: max |diff| {float((x.double() - y.double()).abs().max()):.3e}'


def _assert_against_fp64_and_torch(c, snaps, what):
    """dW against the fp64 sum of the partials, every Adam step against torch.optim.Adam from the state before it (moments
    bit-equal, parameter within 2 ulp of its operands: test_adam_rounding_sequence_and_fused_entry_points), the parameters after
    K steps against torch.optim.Adam fed the fp64-reduced gradients (1e-6: test_adam_matches_torch_optim), the history ring
    and the counters."""
    K = c.K
    hist_prev = torch.full((c.capacity, 4), SENTINEL)
    for k in range(2):
        ref = torch.nn.Parameter(c.p0[k].cpu().clone())
        opt = torch.optim.Adam([ref], lr=HYPER[0], betas=HYPER[1:3], eps=HYPER[3])
        opt.state[ref] = {'step': torch.tensor(float(c.t0)), 'exp_avg': c.m0[k].cpu().clone(), 'exp_avg_sq': c.v0[k].cpu().clone()}
        prev = dict(dw=c.dw0[k].cpu(), p=c.p0[k].cpu(), m=c.m0[k].cpu(), v=c.v0[k].cpu())
        acc64 = c.dw0[k].double().cpu()
        parts = c.parts[k].double().cpu()
        for step in range(K):
            dw, p, m, v = (snaps[step][i * 2 + k] for i in range(4))
            want = parts[step].sum(0) + (prev['dw'].double() if c.acc[k] else 0.0)
            e = rel_l2(dw, want)
            assert e < TOL, f'{what}: dW{k + 1} after step {step + 1} against the fp64 sum of {c.np[k]} partials: {e:.3e}'
            # one Adam step from the state before this launch with the gradient the launch reduced
            one = torch.nn.Parameter(prev['p'].clone())
            o1 = torch.optim.Adam([one], lr=HYPER[0], betas=HYPER[1:3], eps=HYPER[3])
            o1.state[one] = {'step': torch.tensor(float(c.t0 + step)), 'exp_avg': prev['m'].clone(), 'exp_avg_sq': prev['v'].clone()}
            one.grad = dw.clone()
            o1.step()
            assert torch.equal(m, o1.state[one]['exp_avg']), f'{what}: exp_avg{k + 1} after step {step + 1}'
            assert torch.equal(v, o1.state[one]['exp_avg_sq']), f'{what}: exp_avg_sq{k + 1} after step {step + 1}'
            ulp = float(np.spacing(np.float32(max(float(prev['p'].abs().max()), HYPER[0]))))
            assert float((p - one.detach()).abs().max()) <= 2 * ulp, f'{what}: param{k + 1} after step {step + 1} (t = {c.t0 + step + 1})'
            # ... and the K-step trajectory on the fp64-reduced gradients
            acc64 = parts[step].sum(0) + (acc64 if c.acc[k] else 0.0)
            ref.grad = acc64.float()
            opt.step()
            prev = dict(dw=dw, p=p, m=m, v=v)
        e = rel_l2(snaps[-1][2 + k], ref.detach())
        assert e < 1e-6, f'{what}: param{k + 1} after {K} steps against torch.optim.Adam: {e:.3e}'
    lp = [x.double().cpu() for x in c.lp]
    for step in range(K):
        hist, pos, it, arrive = snaps[step][8:12]
        slot = (c.pos0 + step) % c.capacity
        want = [float(lp[j][step, :c.n[j], q].sum()) for j in range(2) for q in range(2)]
        np.testing.assert_allclose(hist[slot].double().numpy(), want, rtol=1e-5, atol=0, err_msg=f'{what}: hist[{slot}] after step {step + 1}')
        others = torch.arange(c.capacity) != slot
        assert torch.equal(hist[others], hist_prev[others]), f'{what}: a history row other than {slot} changed in step {step + 1}'
        hist_prev = hist
        assert int(pos) == (c.pos0 + step + 1) % c.capacity, f'{what}: ring position after step {step + 1}'
        assert int(it) == c.t0 + step + 1, f'{what}: iteration counter after step {step + 1}'
        assert int(arrive[0]) == 0 and int(arrive[1]) == 0, f'{what}: arrive = {arrive.tolist()} after step {step + 1}'


def _compare(c, what=None, by_rows=False):
    what = what or f'd = {c.d}, partials = {c.np}, accumulate = {c.acc}, loss partials = {c.n}, capacity = {c.capacity}, t0 = {c.t0}'
    sep = _run(c, _separate)
    _assert_against_fp64_and_torch(c, sep, what + ' [separate launches]')
    tail = _run(c, _tail)
    _assert_same_bits(tail, sep, what + ' [parts form]')
    _assert_against_fp64_and_torch(c, tail, what + ' [tail launch]')        # (arrive == 0 after every step is asserted here)
    if by_rows:
        rows = _run(c, lambda c_, s_: _tail(c_, s_, by_rows=True))
        _assert_same_bits(rows, sep, what + ' [row-count form]')
        assert all(int(s[11][0]) == 0 and int(s[11][1]) == 0 for s in rows)


WIDTHS = [(128, 64), (64, 128), (64, 64), (32, 32), (128, 128), (6, 10), (2, 2)]
# on both sides of every boundary of the partial loop: `b + 48 < n_part` unrolled by 64, the 16-stride remainder, fewer
# partials than the 16 slices
PART_COUNTS = [1, 2, 15, 16, 17, 48, 49, 63, 64, 65, 127, 128, 129, 256, 512]
ROW_COUNTS = [1, 32, 33, 128, 129, 65_536, 65_537, 70_001]
LOSS_COUNTS = [0, 1, 255, 256, 257, 1000]


@gpu
@pytest.mark.parametrize('d1,d2', WIDTHS)
@pytest.mark.parametrize('np1,np2', [(17, 65), (512, 1), (49, 128)])
def test_tail_launch_at_every_width_pair(d1, d2, np1, np2):
    """(128, 128) is the 513-block grid; (6, 10) and (2, 2) have d d / 4 = 9, 25 and 1 float4 columns - not a multiple of the 16 a
    block owns, the `e4 < n4` guard."""
    _compare(_Case(d1, d2, np1, np2, acc1=0, acc2=1, n1=257, n2=1, capacity=2, K=5, t0=0, seed=d1 + d2 + np1))


@gpu
@pytest.mark.parametrize('n_part', PART_COUNTS)
@pytest.mark.parametrize('d1,d2', [(32, 32), (6, 10), (64, 128)])
def test_tail_launch_at_every_partial_count(n_part, d1, d2):
    other = PART_COUNTS[(PART_COUNTS.index(n_part) + 7) % len(PART_COUNTS)]          # the two weights never share a count
    _compare(_Case(d1, d2, n_part, other, acc1=1, acc2=0, n1=2, n2=256, capacity=3, K=4, t0=3, seed=n_part + d1))


@gpu
@pytest.mark.parametrize('n_sel', ROW_COUNTS)
def test_tail_launch_given_row_counts(n_sel):
    """gd_step_tail_f32 derives the partial count from a row count as the weight-gradient entries do (wgrad_geometry: one
    block up to 32 rows, 32-row steps, at most 512 blocks / 1,024 rows per block)."""
    L = _L()
    other = ROW_COUNTS[(ROW_COUNTS.index(n_sel) + 3) % len(ROW_COUNTS)]
    np1, np2 = L.gd_rows_gemm_wgrad_blocks(n_sel), L.gd_rows_gemm_wgrad_blocks(other)
    assert 1 <= np1 <= 512 and np1 * 1024 >= n_sel
    _compare(_Case(32, 64, np1, np2, acc1=0, acc2=0, n1=L.gd_rowtarget_mse_blocks(n_sel), n2=3, capacity=4, K=3, t0=0, seed=n_sel % 1000,
                   rows=(n_sel, other)), f'n_sel = {n_sel}', by_rows=True)


@gpu
@pytest.mark.parametrize('acc1,acc2', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('t0', [0, 7])
def test_tail_launch_accumulate_flags_and_starting_iteration(acc1, acc2, t0):
    _compare(_Case(128, 64, 70, 33, acc1=acc1, acc2=acc2, n1=4, n2=4, capacity=3, K=4, t0=t0, seed=acc1 * 2 + acc2 + t0))


@gpu
@pytest.mark.parametrize('n1', LOSS_COUNTS)
@pytest.mark.parametrize('n2', LOSS_COUNTS)
def test_tail_launch_loss_partial_counts(n1, n2):
    _compare(_Case(32, 32, 16, 17, n1=n1, n2=n2, capacity=2, K=2, t0=1, seed=n1 + 3 * n2))


@gpu
@pytest.mark.parametrize('capacity,K', [(1, 3), (2, 5), (3, 7), (5, 11)])
def test_history_ring_wraps(capacity, K):
    """K > 2 x capacity: every slot is overwritten at least twice; capacity 1 keeps the position at 0."""
    assert K >= 2 * capacity + 1
    _compare(_Case(64, 64, 20, 3, acc1=1, acc2=1, n1=10, n2=300, capacity=capacity, K=K, t0=2, seed=capacity))


@gpu
def test_two_tails_back_to_back_without_a_host_sync():
    """Nothing between two tail launches on one stream but the copies of the next step's partials (no host round trip:
    _run synchronises once, at the end) - the second launch must see `arrive` reset and the counter advanced by the first.
    Here even those copies are gone: both steps' launches are enqueued back to back on static inputs."""
    c = _Case(128, 64, 129, 64, acc1=1, acc2=0, n1=5, n2=6, capacity=3, K=1, t0=0, seed=5)
    L = _L()
    outs = []
    for launch in (_separate, _tail):
        s = _State(c)
        s.load(c, 0)
        torch.cuda.synchronize()
        for _ in range(6):
            launch(c, s)
        snap = s.snapshot()
        torch.cuda.synchronize()
        outs.append([x.cpu() for x in snap])
    _assert_same_bits([outs[1]], [outs[0]], 'six launches back to back')
    assert int(outs[1][10]) == 6 and int(outs[1][9]) == (c.pos0 + 6) % 3 and outs[1][11].tolist() == [0, 0]
    # accumulate = 1 six times over the same partials: dw0 + 6 x their sum
    want = c.dw0[0].double().cpu() + 6 * c.parts[0][0].double().sum(0).cpu()
    assert rel_l2(outs[1][0], want) < TOL
    assert L.gd_rows_gemm_wgrad_blocks(128 * 129) == 129


@gpu
def test_tail_launch_replayed_from_a_captured_graph():
    """The engine never launches the tail eagerly: it sits at the end of the captured step.  One capture (a single linear
    chain), K replays with fresh partials copied into the static buffers before each = the bits of K eager calls."""
    c = _Case(128, 64, 200, 50, acc1=0, acc2=1, n1=100, n2=300, capacity=2, K=6, t0=0, seed=11)
    eager = _run(c, _tail)
    s = _State(c)
    s.load(c, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _tail(c, s)                                       # (warm-up outside the capture, then back to the initial state)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    s0 = _State(c)
    for dst, src in zip(s.dw + s.p + s.m + s.v + [s.hist, s.pos, s.iter, s.arrive], s0.dw + s0.p + s0.m + s0.v + [s0.hist, s0.pos, s0.iter, s0.arrive]):
        dst.copy_(src)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _tail(c, s)
    snaps = []
    for step in range(c.K):
        s.load(c, step)
        graph.replay()
        snaps.append(s.snapshot())
    torch.cuda.synchronize()
    snaps = [[x.cpu() for x in snap] for snap in snaps]
    _assert_same_bits(snaps, eager, 'graph replay against eager calls')
    assert all(snap[11].tolist() == [0, 0] for snap in snaps)
    _assert_against_fp64_and_torch(c, snaps, 'graph replay')


@gpu
@pytest.mark.parametrize('n1,n2', [(0, 0), (1, 0), (255, 257), (1000, 256)])
@pytest.mark.parametrize('with_extra', [False, True])
def test_loss_finalize_alone(n1, n2, with_extra):
    """gd_loss_finalize_f32 with extra_sums; n1 = n2 = 0 with extra_sums only is the form the multi-GPU engine uses (the
    all-reduced sums arrive in extra_sums)."""
    L = _L()
    g = torch.Generator().manual_seed(n1 + n2)
    capacity, K, t0 = 3, 7, 5
    hist = torch.full((capacity, 4), SENTINEL, device='cuda')
    pos = torch.tensor([2], dtype=torch.int32, device='cuda')
    it = torch.tensor([t0], dtype=torch.int32, device='cuda')
    want = torch.full((capacity, 4), SENTINEL, dtype=torch.float64)
    for step in range(K):
        p1 = torch.rand(max(n1, 1), 2, generator=g) + 0.01
        p2 = torch.rand(max(n2, 1), 2, generator=g) + 0.01
        extra = torch.rand(4, generator=g) * 100.0
        d1, d2, de = p1.cuda(), p2.cuda(), extra.cuda()
        _check(L.gd_loss_finalize_f32(d1.data_ptr(), n1, d2.data_ptr(), n2, de.data_ptr() if with_extra else None, hist.data_ptr(),
                                      capacity, pos.data_ptr(), it.data_ptr(), _stream()), 'gd_loss_finalize_f32')
        row = torch.cat([p1[:n1].double().sum(0), p2[:n2].double().sum(0)]) + (extra.double() if with_extra else 0.0)
        want[(2 + step) % capacity] = row
        np.testing.assert_allclose(hist.double().cpu().numpy(), want.numpy(), rtol=1e-5, atol=0)
        assert int(pos) == (2 + step + 1) % capacity and int(it) == t0 + step + 1


# ------------------------------------------------------------------------------------------------ refusals: no launch

def _err():
    return _L().gd_last_error_string().decode()


def _tail_args(d1=64, d2=64, np1=4, np2=4, n1=1, n2=1, capacity=4, p=256):
    """Arguments of the tail entries with fake, never dereferenced pointers: the argument checks come before any launch."""
    return [p, np1, d1, 0, p, p, p, p, p, np2, d2, 0, p, p, p, p, *HYPER, p, n1, p, n2, p, capacity, p, p, p, None]


@pytest.mark.parametrize('entry', ['gd_step_tail_f32', 'gd_step_tail_parts_f32'])
def test_tail_entries_refuse_what_they_cannot_run(entry):
    fn = getattr(_L(), entry)
    a = _tail_args(256, 256)                               # 1,024 + 1,024 + 1 blocks: not co-resident
    assert fn(*a) == 2 and entry in _err() and 'co-resident' in _err()
    a = _tail_args(128, 256)                               # 256 + 1,024 + 1
    assert fn(*a) == 2 and entry in _err()
    for which in (1, 9):                                   # no partials / no rows for one of the weights
        a = _tail_args()
        a[which] = 0
        assert fn(*a) == 2 and entry in _err()
    for which in (2, 10):                                  # d d not a multiple of 4
        a = _tail_args()
        a[which] = 3
        assert fn(*a) == 2 and entry in _err()
    for which in (0, 4, 5, 6, 7, 8, 12, 13, 14, 15, 20, 22, 24, 26, 27, 28):
        a = _tail_args()
        a[which] = None
        assert fn(*a) == 1 and entry in _err() and 'null' in _err(), which
    a = _tail_args(capacity=0)
    assert fn(*a) == 1 and entry in _err()
    for which in (0, 4, 8, 12):                            # partials / dw are read and written as float4
        a = _tail_args()
        a[which] = 256 + 4
        assert fn(*a) == 3 and entry in _err() and 'unaligned' in _err(), which
    # loss partials may be absent when their count is 0 (passes the checks up to the grid size: refused there, no launch)
    a = _tail_args(256, 256, n1=0, n2=0)
    a[20] = a[22] = None
    assert fn(*a) == 2


def test_loss_finalize_and_reduce_refuse_null_arguments():
    L = _L()
    p = ctypes.c_void_p(256).value
    assert L.gd_loss_finalize_f32(p, 1, p, 1, None, None, 4, p, p, None) == 1 and 'gd_loss_finalize_f32' in _err()
    assert L.gd_loss_finalize_f32(p, 1, p, 1, None, p, 0, p, p, None) == 1
    assert L.gd_loss_finalize_f32(None, 1, p, 1, None, p, 4, p, p, None) == 1 and 'null partials' in _err()
    assert L.gd_rows_gemm_wgrad_reduce_f32(None, 10, 4, 4, p, 0, None, None, None, None, *HYPER, None) == 1
    assert L.gd_rows_gemm_wgrad_reduce_f32(p, 10, 4, 4, p, 0, p, None, None, None, *HYPER, None) == 1 and 'optimizer' in _err()
    assert L.gd_rows_gemm_wgrad_reduce_f32(p, -1, 4, 4, p, 0, None, None, None, None, *HYPER, None) == 2


# ------------------------------------------------------------------------------------------------ small entries

def _unpack(bits, d):
    """[s, n_words] int32 words -> [s, d] bool, bit b of word q = column 32 q + b (gd_rows_gemm_signs_f32's layout)."""
    b = (bits[:, :, None] >> torch.arange(32, dtype=torch.int32)) & 1
    return b.reshape(bits.shape[0], -1)[:, :d].bool()


@gpu
@pytest.mark.parametrize('d', [4, 36, 128])
@pytest.mark.parametrize('n,frac', [(300, 0.6), (70, 1.0), (50, 0.0)])
def test_gate_rows_against_where_on_the_unpacked_bits(d, n, frac):
    """R-GCN's ReLU backward on a row subset: d = 4 (one nibble), 36 (crosses a word: columns 32 .. 35 are the first nibble
    of word 1), 128 (four full words); out of place with a pitched source, in place, dense (idx = NULL), empty list."""
    L = _L()
    g = torch.Generator().manual_seed(d + n)
    n_words = (d + 31) // 32
    mask = torch.rand(n, generator=g) < frac
    idx = mask.nonzero().flatten()
    s = idx.numel()
    bits = torch.randint(-2 ** 31, 2 ** 31, (max(s, 1), n_words), generator=g, dtype=torch.int64).int()
    gate = _unpack(bits, d)[:s]
    ld_src, ld_out = d + 8, d + 4
    src = torch.full((n, ld_src), float('nan'))
    src[:, 4:4 + d] = torch.randn(n, d, generator=g)
    src_g, bits_g, idx_g = src.cuda(), bits.cuda(), idx.int().cuda()
    view = src_g[:, 4:4 + d]
    out = torch.full((n, ld_out), SENTINEL, device='cuda')
    _check(L.gd_gate_rows_f32(view.data_ptr(), ld_src, idx_g.data_ptr(), s, bits_g.data_ptr(), d, out.data_ptr(), ld_out, _stream()),
           'gd_gate_rows_f32')
    want = torch.full((n, ld_out), SENTINEL)
    want[idx, :d] = torch.where(gate, src[idx, 4:4 + d], torch.zeros(()))
    assert torch.equal(out.cpu(), want)                    # selected values exact, pad columns and unlisted rows untouched
    # in place (src == out)
    z = view.contiguous()
    z0 = z.cpu()
    _check(L.gd_gate_rows_f32(z.data_ptr(), d, idx_g.data_ptr(), s, bits_g.data_ptr(), d, z.data_ptr(), d, _stream()), 'gd_gate_rows_f32')
    want = z0.clone()
    want[idx] = torch.where(gate, z0[idx], torch.zeros(()))
    assert torch.equal(z.cpu(), want)
    # dense: idx = NULL gates rows 0 .. n_sel - 1 with bit rows 0 .. n_sel - 1
    if s:
        out = torch.full((n, d), SENTINEL, device='cuda')
        _check(L.gd_gate_rows_f32(view.data_ptr(), ld_src, None, s, bits_g.data_ptr(), d, out.data_ptr(), d, _stream()), 'gd_gate_rows_f32')
        want = torch.full((n, d), SENTINEL)
        want[:s] = torch.where(gate, src[:s, 4:4 + d], torch.zeros(()))
        assert torch.equal(out.cpu(), want)


@gpu
@pytest.mark.parametrize('with_perm', [False, True])
def test_segment_sum_against_fp64(with_perm):
    """Empty segments (also first and last), single entries, one segment of several thousand entries."""
    L = _L()
    g = torch.Generator().manual_seed(3 + with_perm)
    cnt = torch.randint(0, 5, (400,), generator=g)
    cnt[0] = cnt[-1] = cnt[100] = 0
    cnt[37] = 1
    cnt[200] = 5003
    cnt[201] = 64
    cnt[202] = 65
    n = cnt.numel()
    rowptr = torch.zeros(n + 1, dtype=torch.int32)
    rowptr[1:] = cnt.cumsum(0)
    nnz = int(rowptr[-1])
    x = torch.randn(nnz, generator=g)
    perm = torch.randperm(nnz, generator=g).int()
    src = x[perm.long()] if with_perm else x
    seg = torch.repeat_interleave(torch.arange(n), cnt)
    want = torch.zeros(n, dtype=torch.float64).index_add_(0, seg, src.double())
    scale = torch.zeros(n, dtype=torch.float64).index_add_(0, seg, src.double().abs())
    rg, xg, pg = rowptr.cuda(), x.cuda(), perm.cuda()
    outs = []
    for _ in range(2):
        out = torch.full((n,), SENTINEL, device='cuda')
        _check(L.gd_segment_sum_f32(rg.data_ptr(), pg.data_ptr() if with_perm else None, xg.data_ptr(), n, out.data_ptr(), _stream()),
               'gd_segment_sum_f32')
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])                   # fixed order: bit-reproducible
    assert rel_l2(outs[0], want) < TOL
    # per segment: within fp32 summation error of the segment's own magnitude (a hub sum must not hide in the norm, nor a
    # light one behind the hub's); n eps sum |x| is the classical bound of ANY summation order
    eps = float(np.finfo(np.float32).eps)
    assert bool(((outs[0].double() - want).abs() <= cnt.double().clamp(min=1) * eps * scale).all())
    assert bool((outs[0][cnt == 0] == 0).all())
    # n = 0: nothing to do, nothing written
    out = torch.full((4,), SENTINEL, device='cuda')
    assert L.gd_segment_sum_f32(rg.data_ptr(), None, xg.data_ptr(), 0, out.data_ptr(), _stream()) == 0
    assert bool((out == SENTINEL).all())
