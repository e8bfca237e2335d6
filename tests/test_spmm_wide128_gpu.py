"""gd_spmm_csr_onepass_wide128_f32: the 128-float aggregation on the items of the wide form (up to 16 consecutive light rows per
item, two float4 per lane and trip, eight fp32 matrix instructions), hub rows on the vector path of the item kernel inside the same
launch.  On the 2,600-row CSR of spmm_cases.py (light-row runs between 70-edge hubs, hubs from 65 to 5,000 entries, the first row,
the last row behind an empty one) and its transpose, under the full, subset and row-range plans: integer data bit for bit against
the fp64 reference, float data under gamma_k S per element (spmm_cases.hold), y at pitch 144 with sentinel pad columns and sentinel
rows outside the plan, x at pitch 144 too, weights / bias / self term from x and from a separate matrix (the GIN form), hub rows bit
for bit against gd_spmm_csr_onepass_f32, the same bits twice, a grid of 8 blocks (every wave makes at least 3 visits), and the
entry's refusals."""
import pytest
import torch

import spmm_cases as C

pytestmark = pytest.mark.gpu
D = 128
GD_E_DIM = 2


@pytest.fixture(scope='module')
def plans():
    return {(name, direction): C.split_plan(name, direction, 'cuda') for name in C.PLANS for direction in ('fwd', 'bwd')}


@pytest.fixture
def wide_calls(monkeypatch):
    """Calls that reached the wide 128-float entry (the handle of the loaded library is one object per process)."""
    from gnndelete_amd import _lib
    calls = []
    entry = _lib.lib().gd_spmm_csr_onepass_wide128_f32
    monkeypatch.setattr(_lib.lib(), 'gd_spmm_csr_onepass_wide128_f32', lambda *a: calls.append(1) or entry(*a), raising=False)
    return calls


def _raw(direction, plan, **kw):
    from gnndelete_amd import ops
    rowptr, col = C.dev_graph(direction)
    kw.setdefault('wide128', True)                                               # (what the GCN step folded in layer 1 passes)
    return lambda val, x, bias, coef, y, xs: ops._spmm_raw(rowptr, col, val, x, bias, coef, C.N, plan, out=y, x_self=xs, **kw)


def _pitch144(t):
    buf = torch.full((C.N, D + C.PAD), 3.0, device='cuda')
    buf[:, :D] = t
    return buf[:, :D]


def test_wide128_form_on_every_plan_and_both_csrs(plans, wide_calls):
    items, n, b, _ = plans['full', 'fwd'].onepass_wide128()
    for name, degs in C.RUNS.items():                                            # the crafted runs travel as the wide form's items
        assert C.run_items(items, n, C.RUN_START[name], len(degs), form='wide') == C.greedy_rule(degs), name
    assert len(C.group_rows(items, n)) == 26
    worst = 0.0
    for (name, direction), plan in plans.items():
        worst = max(worst, C.hold(_raw(direction, plan), D, name, direction, tag='wide128'))
    assert len(wide_calls) == 6 * 4 * 2                                          # the wide 128-float entry took every call
    for (name, direction) in (('full', 'fwd'), ('subset', 'bwd')):               # x and x_self at pitch 144 as well
        worst = max(worst, C.hold(_raw(direction, plans[name, direction]), D, name, direction, place=_pitch144, tag='wide128 pitch 144'))
    print(f'wide form d=128: bit-exact on integer data, largest |err| / (gamma_k S) on float data {worst:.3f}')


def test_small_grid_every_wave_visits_at_least_three_items(plans, wide_calls, monkeypatch):
    cap = 8
    monkeypatch.setenv('GD_SPMM_GRID_CAP', str(cap))                             # (this launch reads the cap per call)
    worst = 0.0
    for (name, direction), plan in plans.items():
        items, n, b, _ = plan.onepass_wide128()
        # (a range may be empty - the 5,000-entry hub weighs an XCD's share alone - and its waves return at once)
        assert min(v for length, v in C.visits_per_wave(n, b, cap=cap) if length) >= 3, (name, direction)
        if (name, direction) == ('full', 'fwd'):                                 # hub groups on a wave's third visit and later
            visit = C.visit_of_items(n, b, cap=cap)
            assert any(int(visit[i]) >= 2 for i, _, _ in C.group_rows(items, n)) and int(visit.max()) >= 8
        worst = max(worst, C.hold(_raw(direction, plan), D, name, direction, tag=f'wide128 cap {cap}'))
    assert len(wide_calls) == 6 * 4 * 2
    print(f'wide form d=128, grid cap {cap}: bit-exact on integer data, largest |err| / (gamma_k S) on float data {worst:.3f}')


def test_hub_rows_carry_the_item_kernels_bits_and_runs_repeat(plans, wide_calls):
    for (name, direction), plan in plans.items():
        rows, _ = C.dev_plan_rows(name)
        hubs = rows[(C.degrees(direction).cuda()[rows] > C.CHUNK)]
        assert hubs.numel() >= 5 or direction == 'bwd'                           # (the transposed CSR has no row above 64 entries)
        for option in (0, 2, 3):                                                 # weights + bias; + 0.5 x_self; unweighted + bias + x
            weighted, with_bias, coef, src = C.OPTIONS[option]
            val = C.dev_values('float', C.val_name('float', option), direction)
            x, xs = C.dev_rows('float', 'x', D), (C.dev_rows('float', 'xs', D) if src == 'xs' else None)
            bias = C.dev_rows('float', 'b', D) if with_bias else None
            out = []
            for kw in ({}, {}, {'wide128': False}):
                yb = torch.full((C.N, D + C.PAD), C.SENTINEL, device='cuda')
                before = len(wide_calls)
                _raw(direction, plan, **dict(kw))(val, x, bias, coef, yb[:, :D], xs)
                assert len(wide_calls) - before == (0 if 'wide128' in kw else 1)
                out.append(yb)
            assert torch.equal(out[0], out[1]), (name, direction, option, 'two runs differ')
            assert torch.equal(out[0][hubs], out[2][hubs]), (name, direction, option, 'a hub row differs from gd_spmm_csr_onepass_f32')


def test_wide128_entry_checks_its_arguments(plans):
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import ptr
    plan = plans['full', 'fwd']
    items, n_items, bounds, tags = plan.onepass_wide128()
    col = C.dev_graph('fwd')[1]
    colt = col | (tags << 24)
    x = torch.zeros(C.N, D, device='cuda')
    y = torch.zeros(C.N, D, device='cuda')

    def call(d, x_rows, n_it=n_items, yy=y):
        return _lib.lib().gd_spmm_csr_onepass_wide128_f32(ptr(items), n_it, ptr(colt), None, ptr(x), D, ptr(yy), D, None, 0.0, None, d,
                                                          int(colt.shape[0]), x_rows, ptr(bounds), None)
    assert call(64, C.N) == GD_E_DIM and call(132, C.N) == GD_E_DIM and call(256, C.N) == GD_E_DIM     # d must be 128
    assert call(D, 0) == GD_E_DIM and call(D, 1 << 24) == GD_E_DIM               # row ids below 2^24
    assert call(D, C.N, yy=x) == GD_E_DIM                                        # y aliasing x
    assert call(D, C.N, n_it=n_items - 1) == GD_E_DIM                            # an item count that is no multiple of 4
    assert call(D, C.N, n_it=0) == 0
