"""Every form of the GCN / GIN / SAGE aggregation (csrc/spmm.hip) on the crafted CSR of tests/spmm_cases.py, row by row: the
one-wave-per-row vector kernel and its scalar fallback, the one-launch item kernel at every width instantiation (whole rows,
multi-row items with counts of exactly 64 and empty rows, 4-wave groups from 65 to 5000 in-edges), the two-launch piece form,
the 16-row matrix-instruction form, the 64-bit addressing instantiations, the top of the 24-bit path and later visits of a wave
(grid cap 8).  Integer data must equal the fp64 reference BIT FOR BIT on the plan's rows; float data stays per element under
gamma_k S (k = in-degree + 2, derived in spmm_cases, never measured); rows outside the plan and pad columns keep a sentinel.

Largest |err| / (gamma_k S) on the float data per form, as printed with -s on an MI355X (integer data bit-exact everywhere):
    plain entry     vector kernel, d = 4 .. 1024: 0.736    scalar kernel (d = 7, 1028, pitch 10, base off by one float): 0.736
    item kernel     16 widths x 3 plans x forward / transposed: 0.724 (d = 36, 64: two rows per item)
    two-launch      d = 8, 64, 128, 260, also with hand-made range limits: 0.694
    wide form       d = 64, grid cap 8192 and 8: 0.663
    64-bit          onepass entry 0.724, balanced entry 0.640 - the bits of the 24-bit launches
    24-bit top      pitch 4,194,300 floats: item kernel 0.542, wide form 0.495 (a 255-row graph of its own)
    later visits    grid cap 8 in a child process: one-launch 0.724, two-launch 0.694
The fp32 restatements on the host (test_spmm_cases_cpu.py) reach 0.724: the kernels use the bound as fp32 arithmetic does.
"""
import os
import subprocess
import sys

import pytest
import torch

import spmm_cases as C

pytestmark = pytest.mark.gpu
VECTOR_WIDTHS = (4, 8, 12, 16, 32, 64, 68, 128, 132, 256, 260, 512, 516, 1024)
ITEM_WIDTHS = (4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 512, 516, 1024)
GD_E_DIM = 2


@pytest.fixture(scope='module')
def plans():
    return {(name, direction): C.split_plan(name, direction, 'cuda') for name in C.PLANS for direction in ('fwd', 'bwd')}


def _raw(direction, plan, **kw):
    from gnndelete_amd import ops
    rowptr, col = C.dev_graph(direction)
    return lambda val, x, bias, coef, y, xs: ops._spmm_raw(rowptr, col, val, x, bias, coef, C.N, plan, out=y, x_self=xs, **kw)


def _report(form, ratio):
    print(f'{form}: bit-exact on integer data, largest |err| / (gamma_k S) on float data {ratio:.3f}')


def _assert_crafted_items(plan, d):
    """The full forward plan carries the multi-row and group items of the case file at this width."""
    items, n, _ = plan.onepass(d)
    maxr = C.max_rows(d)
    for name, degs in C.RUNS.items():
        assert C.run_items(items, n, C.RUN_START[name], len(degs)) == C.packed_rule(degs, maxr), (d, name)
    assert sorted(r for _, r, _ in C.group_rows(items, n)) == sorted(r for r, k in enumerate(C.DEG.tolist()) if k > 64)
    return items, n


# ----------------------------------------------------------------------------------------------------------- plain entry
@pytest.mark.parametrize('d', VECTOR_WIDTHS)
def test_plain_entry_vector_widths(d):
    worst = max(C.hold(_raw(direction, None), d, 'full', direction, options=C.PLAIN_OPTIONS, tag='vec') for direction in ('fwd', 'bwd'))
    _report(f'plain entry, vector kernel d={d}', worst)


def test_plain_entry_scalar_fallback():
    def pitch10(t):
        buf = torch.full((C.N, 10), 3.0, device='cuda')
        buf[:, :8] = t
        return buf[:, :8]

    def off_by_one_float(t):
        flat = torch.full((C.N * 8 + 1,), 3.0, device='cuda')
        v = flat[1:].view(C.N, 8)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    for tag, d, place in (('d=7', 7, None), ('d=1028', 1028, None), ('d=8 at pitch 10', 8, pitch10), ('d=8 off by one float', 8, off_by_one_float)):
        worst = max(C.hold(_raw(direction, None), d, 'full', direction, options=C.PLAIN_OPTIONS, place=place, tag=tag) for direction in ('fwd', 'bwd'))
        _report(f'plain entry, scalar kernel {tag}', worst)


# ----------------------------------------------------------------------------------------------------- one-launch item kernel
@pytest.mark.parametrize('d', ITEM_WIDTHS)
def test_item_kernel(plans, d):
    _assert_crafted_items(plans['full', 'fwd'], d)
    worst = 0.0
    for (name, direction), plan in plans.items():
        worst = max(worst, C.hold(_raw(direction, plan, wide=False), d, name, direction, tag='items'))
    _report(f'item kernel d={d} (rows per item {C.max_rows(d)}; full / subset / range plans, forward and transposed)', worst)


def test_one_wrong_edge_in_a_table_is_seen_on_the_device(plans):
    """The check has teeth: a table with ONE edge of the 5000-edge hub row dropped and ONE count of a two-row item off by one (its
    33rd edge summed into the row before) changes exactly those three rows of the integer result, and no other."""
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import ptr
    d = 8
    plan = plans['full', 'fwd']
    items, n, bounds = plan.onepass(d)
    bad = items.clone()
    rows, slots, ends = bad[:n, 0].tolist(), bad[:n, 3].tolist(), (bad[:n, 2] - bad[:n, 1]).tolist()
    pair = next(i for i in range(n) if rows[i] == C.RUN_START['32_32'] and slots[i] <= -16)
    bad[pair, 3] -= 1                                                            # b1 = 33
    member = [i for i in range(n) if rows[i] == 1900 and slots[i] == -2 and ends[i] > 0][-1]
    bad[member, 2] -= 1                                                          # the hub's last edge
    col = C.dev_graph('fwd')[1]
    val, x, b = C.dev_values('int', 'w', 'fwd'), C.dev_rows('int', 'x', d), C.dev_rows('int', 'b', d)
    ref = C.dev_reference('int', 0, 'fwd')[0][:, :d]
    for table, want in ((items, []), (bad, [C.RUN_START['32_32'], C.RUN_START['32_32'] + 1, 1900])):
        y = torch.full((C.N, d), C.SENTINEL, device='cuda')
        _lib.check(_lib.lib().gd_spmm_csr_onepass_f32(ptr(table), n, ptr(col), ptr(val), ptr(x), d, ptr(y), d, ptr(b), 0.0, None, d, int(col.shape[0]), C.N,
                                                      ptr(bounds), _lib.stream_ptr(x.device)), 'gd_spmm_csr_onepass_f32')
        assert (y.double() != ref).any(1).nonzero().flatten().tolist() == want


# ------------------------------------------------------------------------------------------------------------ two-launch form
@pytest.mark.parametrize('d', (8, 64, 128, 260))
def test_two_launch_form(plans, d, monkeypatch):
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import ptr
    monkeypatch.setenv('GD_SPMM_TWO_LAUNCH', '1')
    worst = 0.0
    for (name, direction), plan in plans.items():
        assert plan.n_split == int((C.degrees(direction)[C.plan_rows(name)] > 64).sum())
        worst = max(worst, C.hold(_raw(direction, plan), d, name, direction, tag='two-launch'))
    # through the C ABI with range limits that are no multiples of 4 and two empty ranges (the piece form takes them)
    for name in ('full', 'subset'):
        plan = plans[name, 'fwd']
        n = plan.n_items
        odd = lambda v: v if v % 4 else v + 1
        b = [0, 5, 5, odd(n // 3), odd(n // 3), odd(n // 2), odd(2 * n // 3), odd(5 * n // 6), n]
        assert b == sorted(b) and sum(v % 4 != 0 for v in b[1:8]) == 7
        bounds = torch.tensor(b, dtype=torch.int32, device='cuda')
        col = C.dev_graph('fwd')[1]
        scratch = plan.scratch(d, 'cuda')

        def launch(val, x, bias, coef, y, xs):
            _lib.check(_lib.lib().gd_spmm_csr_balanced_f32(ptr(plan.items), n, ptr(plan.split), plan.n_split, ptr(col), ptr(val), ptr(x), x.stride(0),
                                                           ptr(y), y.stride(0), ptr(bias), float(coef), ptr(xs), ptr(scratch), d, int(col.shape[0]), C.N,
                                                           ptr(bounds), _lib.stream_ptr(x.device)), 'gd_spmm_csr_balanced_f32')
        worst = max(worst, C.hold(launch, d, name, 'fwd', tag='two-launch, hand-made ranges'))
    _report(f'two-launch piece form d={d}', worst)


# ------------------------------------------------------------------------------------------------------------------ wide form
def test_wide_form(plans, monkeypatch):
    from gnndelete_amd import ops
    calls = []
    wide_col = ops._wide_col
    monkeypatch.setattr(ops, '_wide_col', lambda *a: calls.append(1) or wide_col(*a))
    items, n, b, _ = plans['full', 'fwd'].onepass_wide(64)
    for name, degs in C.RUNS.items():
        assert C.run_items(items, n, C.RUN_START[name], len(degs), form='wide') == C.greedy_rule(degs), name
    assert len(C.group_rows(items, n)) == 26
    for cap in (None, 8):
        if cap is not None:
            # (this launch reads the cap per call; the item kernel reads it once per process and is not launched here)
            monkeypatch.setenv('GD_SPMM_GRID_CAP', str(cap))
            visit = C.visit_of_items(n, b, cap=cap)
            late_groups = [r for i, r, _ in C.group_rows(items, n) if int(visit[i]) >= 2]
            first_rows = items[:n, 0].tolist()
            crafted = [name for name in C.RUNS if any(int(visit[i]) >= 2 for i in range(n) if first_rows[i] == C.RUN_START[name])]
            assert late_groups and crafted, (late_groups, crafted)
            assert int(visit.max()) >= 8
        worst, before = 0.0, len(calls)
        for (name, direction), plan in plans.items():
            worst = max(worst, C.hold(_raw(direction, plan), 64, name, direction, tag=f'wide cap {cap}'))
        assert len(calls) - before == 6 * 4 * 2                                  # the wide entry took every call
        _report(f'wide form d=64, grid cap {cap or 8192}', worst)


# ---------------------------------------------------------------------------------------------------------- 64-bit addressing
@pytest.mark.parametrize('d', (8, 64, 128, 260))
def test_64_bit_addressing_gives_the_bits_of_the_24_bit_launch(plans, d):
    """x_rows is an upper bound the caller claims: 2^24 + 1 selects the ADDR32 = false instantiations (both EXACT values over the
    four widths), 2^24 is the last value on the fast path."""
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import ptr
    L = _lib.lib()
    col = C.dev_graph('fwd')[1]
    nnz = int(col.shape[0])
    for entry in ('onepass', 'balanced'):
        for name in ('full', 'subset'):
            plan = plans[name, 'fwd']
            seen = {}

            def launcher(x_rows):
                def launch(val, x, bias, coef, y, xs):
                    if entry == 'onepass':
                        items, n, bounds = plan.onepass(d)
                        rc = L.gd_spmm_csr_onepass_f32(ptr(items), n, ptr(col), ptr(val), ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(bias), float(coef),
                                                       ptr(xs), d, nnz, x_rows, ptr(bounds), _lib.stream_ptr(x.device))
                    else:
                        rc = L.gd_spmm_csr_balanced_f32(ptr(plan.items), plan.n_items, ptr(plan.split), plan.n_split, ptr(col), ptr(val), ptr(x),
                                                        x.stride(0), ptr(y), y.stride(0), ptr(bias), float(coef), ptr(xs), ptr(plan.scratch(d, 'cuda')), d,
                                                        nnz, x_rows, None, _lib.stream_ptr(x.device))
                    _lib.check(rc, entry)
                    seen.setdefault(x_rows, []).append(y.clone())
                return launch
            worst = 0.0
            for x_rows in (C.N, (1 << 24) + 1, 1 << 24):
                worst = max(worst, C.hold(launcher(x_rows), d, name, 'fwd', tag=f'{entry} x_rows={x_rows}'))
            for x_rows in ((1 << 24) + 1, 1 << 24):
                assert len(seen[x_rows]) == 8 and all(torch.equal(a, b) for a, b in zip(seen[C.N], seen[x_rows])), (entry, name, x_rows)
            _report(f'64-bit addressing, {entry} entry d={d} {name} plan (bits of the 24-bit launch)', worst)


# ------------------------------------------------------------------------------------------------- the top of the 24-bit path
def _small_graph():
    n = 255
    g = torch.Generator().manual_seed(255)
    deg = torch.randint(0, 9, (n,), generator=g)
    deg[3], deg[100], deg[129], deg[200], deg[254] = 65, 300, 64, 129, 70
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n, (int(deg.sum()),), generator=g)
    order = torch.argsort(dst * n + src, stable=True)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(deg, 0)]).to(torch.int32)
    return n, deg, rowptr, src[order].to(torch.int32).contiguous(), g


def test_top_of_the_24_bit_path():
    """A row pitch just under 2^24 bytes: __umul24(row, pitch) crosses 2^31 at row 129 and reaches 2^32 - 2^24 at the last row.  The
    same graph at a pitch of exactly 2^24 bytes must take the 64-bit instantiation and give the same bits."""
    from gnndelete_amd import _lib, ops
    from gnndelete_amd._lib import ptr
    from gnndelete_amd.graph import SplitPlan
    n, deg, rowptr, col, g = _small_graph()
    assert int((col >= 129).sum()) > 100 and 129 * 4194300 * 4 > 2 ** 31
    nnz = int(col.shape[0])
    rows_of = torch.repeat_interleave(torch.arange(n), deg)
    val = {'int': torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (nnz,), generator=g)], 'float': torch.rand(nnz, generator=g) + 0.25}
    xd = {'int': torch.randint(-8, 9, (n, 128), generator=g).float(), 'float': torch.randn(n, 128, generator=g)}
    bd = {'int': torch.randint(-8, 9, (128,), generator=g).float(), 'float': torch.randn(128, generator=g)}
    rowptr_d, col_d = rowptr.cuda(), col.cuda()
    plan = SplitPlan(rowptr_d)
    assert len(C.group_rows(*plan.onepass(8)[:2])) == 4 and len(C.group_rows(*plan.onepass_wide(64)[:2])) == 4
    gam = C.gamma(deg + 2)[:, None]
    buf = torch.empty(255 * 4194304, dtype=torch.float32, device='cuda')             # 4.3 GB, uninitialised
    try:
        worst = {}
        for d, forms in ((8, ('items',)), (128, ('items',)), (64, ('items', 'wide'))):
            for weighted, with_bias, coef in ((True, True, 1.0), (False, False, 0.5)):
                for kind in ('int', 'float'):
                    x, b = xd[kind][:, :d], (bd[kind][:d] if with_bias else None)
                    w = val[kind] if weighted else None
                    ref = C.aggregate(rowptr, col, w, x, torch.float64) + coef * x.double() + (b.double() if with_bias else 0.0)
                    s = C.aggregate(rowptr, col, w, x.abs(), torch.float64) + coef * x.double().abs() + (b.double().abs() if with_bias else 0.0)
                    out = {}
                    for pitch in (4194300, 4194304):
                        xv = buf[:n * pitch].view(n, pitch)[:, :d]
                        xv.copy_(x.cuda())
                        assert xv.stride(0) * 4 * (n - 1) + 4 * d <= buf.numel() * 4
                        for form in forms:
                            if pitch == 4194304 and form == 'wide':
                                continue
                            yb = torch.full((n, d + C.PAD), C.SENTINEL, device='cuda')
                            ops._spmm_raw(rowptr_d, col_d, None if w is None else w.cuda(), xv, None if b is None else b.cuda(), coef, n, plan,
                                          out=yb[:, :d], wide=(form == 'wide'))
                            y = yb[:, :d].cpu()
                            assert bool((yb[:, d:] == C.SENTINEL).all())
                            if kind == 'int':
                                assert torch.equal(y.double(), ref), (d, form, pitch, coef)
                            else:
                                ratio = C.error_ratio(y, ref, gam * s)
                                assert ratio <= 1.0, (d, form, pitch, ratio)
                                worst[form] = max(worst.get(form, 0.0), ratio)
                            out[form, pitch] = y
                    assert torch.equal(out['items', 4194300], out['items', 4194304]), (d, kind, 'the 64-bit instantiation gives other bits')
        # the wide entry refuses the pitch of 2^24 bytes
        items, n_items, bounds, tags = plan.onepass_wide(64)
        colt = col_d | (tags << 24)
        xv = buf[:n * 4194304].view(n, 4194304)[:, :64]
        y = torch.zeros(n, 64, device='cuda')
        rc = _lib.lib().gd_spmm_csr_onepass_wide_f32(ptr(items), n_items, ptr(colt), None, ptr(xv), 4194304, ptr(y), 64, None, 0.0, None, 64, nnz, n,
                                                     ptr(bounds), None)
        assert rc == GD_E_DIM
        for form, ratio in worst.items():
            _report(f'top of the 24-bit path (pitch 4,194,300 floats), {"item kernel d=8/64/128" if form == "items" else "wide form d=64"}', ratio)
    finally:
        del buf
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- edgeless graphs
def test_item_entries_refuse_items_without_edges(plans):
    """n_items > 0 with nnz <= 0 is GD_E_DIM in every item entry (the index prefetch clamps to nnz - 1): no launch."""
    from gnndelete_amd import _lib
    from gnndelete_amd._lib import ptr
    L = _lib.lib()
    plan = plans['full', 'fwd']
    items, n, bounds = plan.onepass(64)
    witems, wn, wbounds, _ = plan.onepass_wide(64)
    col = torch.zeros(64, dtype=torch.int32, device='cuda')                       # a non-NULL dummy
    x, y = torch.zeros(C.N, 64, device='cuda'), torch.full((C.N, 64), C.SENTINEL, device='cuda')
    aux, aux_sum = torch.zeros(64, 2, device='cuda'), torch.zeros(C.N, device='cuda')
    for nnz in (0, -1):
        assert L.gd_spmm_csr_onepass_f32(ptr(items), n, ptr(col), None, ptr(x), 64, ptr(y), 64, None, 0.0, None, 64, nnz, C.N, ptr(bounds), None) == GD_E_DIM
        assert L.gd_spmm_csr_onepass_wide_f32(ptr(witems), wn, ptr(col), None, ptr(x), 64, ptr(y), 64, None, 0.0, None, 64, nnz, C.N, ptr(wbounds),
                                              None) == GD_E_DIM
        assert L.gd_spmm_csr_balanced_f32(ptr(plan.items), plan.n_items, ptr(plan.split), plan.n_split, ptr(col), None, ptr(x), 64, ptr(y), 64, None, 0.0,
                                          None, ptr(plan.scratch(64, 'cuda')), 64, nnz, C.N, None, None) == GD_E_DIM
        assert L.gd_spmm_csr_onepass_aux_f32(ptr(items), n, ptr(col), ptr(col), ptr(aux), ptr(x), 64, ptr(y), 64, ptr(aux_sum), 64, nnz, C.N, ptr(bounds),
                                             None) == GD_E_DIM
    assert b'without entries' in L.gd_last_error_string()
    torch.cuda.synchronize()
    assert bool((y == C.SENTINEL).all())
    # no items: nothing to do, with or without edges
    assert L.gd_spmm_csr_onepass_f32(ptr(items), 0, ptr(col), None, ptr(x), 64, ptr(y), 64, None, 0.0, None, 64, 0, C.N, ptr(bounds), None) == 0


@pytest.mark.parametrize('mode', ['sum', 'mean'])
def test_aggregation_over_an_edgeless_graph(mode):
    """GINConv / SAGEConv on an edge list without edges: y = self_coef x + bias, and the gradient of x is self_coef dy."""
    from gnndelete_amd import ops
    from gnndelete_amd.graph import SplitPlan, build_csr
    n, d = 37, 64
    gr = build_csr(torch.zeros(2, 0, dtype=torch.long, device='cuda'), n, mode)
    assert gr.nnz == 0 and int(gr.rowptr.abs().max()) == 0
    g = torch.Generator().manual_seed(37)
    x, b = torch.randn(n, d, generator=g).cuda().requires_grad_(), torch.randn(d, generator=g).cuda()
    for coef in (0.0, 1.0, 0.5):
        y = ops.spmm(x, gr, b, coef)
        assert torch.equal(y, x.detach() * coef + b)
        dy = torch.randn(n, d, generator=g).cuda()
        dx, = torch.autograd.grad(y, x, dy)
        assert torch.equal(dx, dy * coef)
    y = ops.spmm(x.detach(), gr, None, 0.0)
    assert bool((y == 0).all())
    rows = torch.tensor([0, 5, 6, 36], device='cuda')
    out = torch.full((n, d), C.SENTINEL, device='cuda')
    xs = torch.randn(n, d, generator=g).cuda()
    ops._spmm_raw(gr.rowptr, gr.col, gr.val, x.detach(), b, 0.5, n, SplitPlan(gr.rowptr, rows=rows), out=out, x_self=xs)
    keep = torch.ones(n, dtype=torch.bool, device='cuda')
    keep[rows] = False
    assert torch.equal(out[rows], xs[rows] * 0.5 + b) and bool((out[keep] == C.SENTINEL).all())


# ----------------------------------------------------------------------------------------- later visits of the item kernel
def test_later_visits_of_the_item_kernel():
    """The item kernel reads its grid cap once per process: ONE fresh child with GD_SPMM_GRID_CAP=8 (8 blocks, 4 waves per XCD, every
    wave at least 3 visits) holds both plans at five widths, one-launch and two-launch, to the same checks."""
    env = dict(os.environ, GD_SPMM_GRID_CAP='8')
    env.pop('GD_SPMM_TWO_LAUNCH', None)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'spmm_visits_worker.py')
    res = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=240)
    print(res.stdout[-4000:])
    assert res.returncode == 0 and 'SPMM_VISITS_OK' in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
