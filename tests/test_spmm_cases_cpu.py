"""The case file of the SpMM form tests (tests/spmm_cases.py) checked on the host: the crafted CSR and its three plans have the
items they were built for, every item table covers every edge of the planned rows exactly once and no other, the host walkers
reproduce the fp64 reference bit for bit on the integer data - and do NOT with one deliberate mis-decode each, so the case can
tell the difference - the integer data is exact in fp32 in any order, and the fp32 restatements stay inside the gamma_k bound on
the float data.  No GPU."""
import pytest
import torch

import spmm_cases as C

WIDTH_OF = {4: 8, 2: 64, 1: 128}          # a width whose item kernel decodes that many rows per item


@pytest.fixture(scope='module')
def plans():
    return {(name, direction): C.split_plan(name, direction) for name in C.PLANS for direction in ('fwd', 'bwd')}


def test_degrees_and_runs_are_the_crafted_ones():
    deg = C.degrees('fwd')
    assert torch.equal(deg, C.DEG) and int(deg[0]) == 65 and int(deg[C.N - 2]) == 0 and int(deg[C.N - 1]) == 130
    assert int(deg[700]) == 192 and int(deg[701]) == 193 and int(deg[900]) == 256 and int(deg[901]) == 257      # side by side
    for name, degs in {**C.RUNS, **C.LATE_RUNS}.items():
        r = C.RUN_START[name]
        assert deg[r:r + len(degs)].tolist() == degs and int(deg[r - 1]) == C.SEP and int(deg[r + len(degs)]) == C.SEP, name
    assert sorted(int(v) for v in deg[deg > 64].unique()) == sorted({65, 70, 128, 129, 130, 192, 193, 256, 257, 320, 321, 1025, 5000})
    assert int(C.degrees('bwd').sum()) == int(deg.sum())


def test_full_plan_has_the_items_the_runs_were_built_for(plans):
    p = plans['full', 'fwd']
    want4 = {'64_0_0_0': [(0, 4, (64, 64, 64), 64)], '0_0_0_64': [(0, 4, (0, 0, 0), 64)], '0_0_0_0': [(0, 4, (0, 0, 0), 0)],
             '16x4': [(0, 4, (16, 32, 48), 64)], '16_16_16_17': [(0, 1, (), 16), (1, 1, (), 16), (2, 1, (), 16), (3, 1, (), 17)],
             '1_62_1': [(0, 3, (1, 63), 64)], '32_32': [(0, 2, (32,), 64)], '32_33': [(0, 1, (), 32), (1, 1, (), 33)],
             '0_64': [(0, 2, (0,), 64)], '64_0': [(0, 2, (64,), 64)]}
    want2 = {'16x4': [(0, 2, (16,), 32), (2, 2, (16,), 32)], '64_0_0_0': [(0, 2, (64,), 64), (2, 2, (0,), 0)],
             '0_0_0_64': [(0, 2, (0,), 0), (2, 2, (0,), 64)], '16_16_16_17': [(0, 2, (16,), 32), (2, 2, (16,), 33)],
             '1_62_1': [(0, 2, (1,), 63), (2, 1, (), 1)]}
    for multirow in (4, 2, 1):
        items, n, _ = p.onepass(WIDTH_OF[multirow])
        for name, degs in {**C.RUNS, **C.LATE_RUNS}.items():
            got = C.run_items(items, n, C.RUN_START[name], len(degs))
            assert got == C.packed_rule(degs, multirow), (multirow, name, got)
            if multirow == 4 and name in want4:
                assert got == want4[name], (name, got)
            if multirow == 2 and name in want2:
                assert got == want2[name], (name, got)
            if multirow == 1:
                assert got == [(q, 1, (), g) for q, g in enumerate(degs)]
    items, n, _, tags = p.onepass_wide(64)
    for name, degs in C.RUNS.items():
        assert C.run_items(items, n, C.RUN_START[name], len(degs), form='wide') == C.greedy_rule(degs), name
    assert C.run_items(items, n, C.RUN_START['16_16_16_17'], 4, form='wide') == [(0, 3, None, 48), (3, 1, None, 17)]


def test_group_quadruples(plans):
    hubs = {r: int(k) for r, k in enumerate(C.DEG.tolist()) if k > 64}
    assert len(hubs) == 26
    for d in (8, 64, 128):
        for form in ('onepass', 'wide'):
            if form == 'wide' and d != 64:
                continue
            tab = plans['full', 'fwd'].onepass(d) if form == 'onepass' else plans['full', 'fwd'].onepass_wide(64)
            items, n, b = tab[0], tab[1], tab[2].tolist()
            groups = C.group_rows(items, n)
            assert sorted(r for _, r, _ in groups) == sorted(hubs)
            share = {r: m for _, r, m in groups}
            for r, k in hubs.items():
                pieces = (k + 63) // 64
                s = 64 * ((pieces + 3) // 4)
                assert share[r] == [max(0, min(s, k - w * s)) for w in range(4)], (r, share[r])
            assert share[0] == [64, 1, 0, 0] and share[900] == [64, 64, 64, 64] and share[901] == [128, 128, 1, 0]
            assert share[1900] == [1280, 1280, 1280, 1160] and share[1500] == [320, 320, 320, 65]
            # the rows above 4 pieces come first in their range, heaviest first; every other group after a light row or a group
            at = {r: i for i, r, _ in groups}
            for k in range(8):
                big = [r for r in C.BIG if b[k] <= at[r] < b[k + 1]]
                assert [at[r] for r in big] == [b[k] + 4 * j for j in range(len(big))], (d, form, k, big)
            assert sorted(C.BIG) == sorted(r for r, v in hubs.items() if v > 256)
    groups = C.group_rows(*plans['subset', 'fwd'].onepass(8)[:2])
    assert sorted(r for _, r, _ in groups) == sorted(int(r) for r in C.plan_rows('subset') if int(C.DEG[r]) > 64) and len(groups) == 11


def test_subset_and_range_plans_cut_the_runs(plans):
    r = C.RUN_START
    sub, rng = plans['subset', 'fwd'], plans['range', 'fwd']
    for multirow, want in ((4, [(0, 2, (16,), 32), (3, 1, (), 16)]), (2, [(0, 2, (16,), 32), (3, 1, (), 16)]), (1, [(0, 1, (), 16), (1, 1, (), 16), (3, 1, (), 16)])):
        items, n, _ = sub.onepass(WIDTH_OF[multirow])
        assert C.run_items(items, n, r['16x4'], 4) == want                   # rows 0, 1, 3 of the run: a pair, then a single
    items, n, _ = sub.onepass(8)
    assert C.run_items(items, n, r['64_0_0_0'], 4) == [(1, 3, (0, 0), 0)]    # three rows without an edge: cnt = 0
    assert C.run_items(items, n, r['0_0_0_64'], 4) == [(0, 1, (), 0), (3, 1, (), 64)]
    assert C.run_items(items, n, r['1_62_1'], 3) == [(0, 2, (1,), 63)]       # cut by the gap behind it
    assert C.run_items(items, n, r['64_0'], 2) == [(0, 2, (64,), 64)]        # cut by the hub behind it
    items, n, _ = sub.onepass(64)
    assert C.run_items(items, n, r['64_0_0_0'], 4) == [(1, 2, (0,), 0), (3, 1, (), 0)]
    items, n, _, _ = sub.onepass_wide(64)
    assert C.run_items(items, n, r['16x4'], 4, form='wide') == [(0, 2, None, 32), (3, 1, None, 16)]
    # the row range starts at the second row of a run and ends behind the second row of another
    items, n, _ = rng.onepass(8)
    assert C.run_items(items, n, r['16x4'], 4) == [(1, 3, (16, 32), 48)]
    assert C.run_items(items, n, r['late_16x4'], 4) == [(0, 2, (16,), 32)]
    assert int(items[:n, 0].max()) == r['late_16x4'] and int(items[:n][items[:n, 0] >= 0][:, 0].min()) == r['16x4'] + 1
    items, n, _ = rng.onepass(64)
    assert C.run_items(items, n, r['16x4'], 4) == [(1, 2, (16,), 32), (3, 1, (), 16)]


@pytest.mark.parametrize('direction', ['fwd', 'bwd'])
@pytest.mark.parametrize('name', C.PLANS)
def test_every_table_covers_the_planned_edges_once(plans, name, direction):
    p = plans[name, direction]
    rp = C.graph()[direction][0].long()
    true_row = C.row_of_entry(direction)
    planned = torch.zeros(C.N, dtype=torch.bool)
    planned[C.plan_rows(name)] = True
    tables = [('onepass', WIDTH_OF[m], p.onepass(WIDTH_OF[m], multirow=m)) for m in (4, 2, 1)]
    tables += [('wide', 64, p.onepass_wide(64)), ('pieces', 8, (p.items, p.n_items, None))]
    for form, d, tab in tables:
        items, n, b = tab[0], tab[1], tab[2]
        if b is not None:
            b = b.tolist()
            assert b[0] == 0 and b[8] == n and all(v % 4 == 0 for v in b) and b == sorted(b) and n % 4 == 0, (form, b)
            assert all(i % 4 == 0 for i, _, _ in C.group_rows(items, n))
            assert int((items[:n, 3] == -2).sum()) == 4 * len(C.group_rows(items, n))
            for i, _, _ in C.group_rows(items, n):                            # no quadruple straddles a range limit
                assert any(b[k] <= i and i + 4 <= b[k + 1] for k in range(8))
        ent, rows = C.item_edges(items, n, form, d, tab[3] if form == 'wide' else None)
        count = torch.bincount(ent, minlength=int(rp[-1]))
        assert torch.equal(count, planned[true_row].long()), (form, 'an edge covered twice, not at all, or of a row outside the plan')
        assert torch.equal(rows, true_row[ent]), (form, 'an edge summed into another row')
        # every planned row is written by exactly one item (rows without an edge included)
        written = torch.zeros(C.N, dtype=torch.long)
        for row, start, end, slot in items[:n].tolist():
            if row < 0:
                continue
            if form == 'wide' and slot != -2:
                written[row:row + (-slot - 15)] += 4
            elif form == 'onepass' and slot <= -16:
                written[row:row + C.decode_multi(slot, 4)[0]] += 4
            elif slot == -2 or slot >= 0:
                written[row] += 1 if slot == -2 else 0
            else:
                written[row] += 4
        if form == 'pieces':
            written[p.split[:, 0].long()] += 4
            assert int(p.split[:, 2].sum()) == p.n_slots == int((items[:, 3] >= 0).sum())
        assert torch.equal(written, 4 * planned.long()), form


def _y0(d):
    return torch.full((C.N, d), 7.0)


def _walk(p, form, kind, option, direction, d, dtype=torch.float64, mis=None):
    col, val, x, xs, bias, coef = C.operands(kind, option, direction, d)
    if form == 'wide':
        items, n, b, tags = p.onepass_wide(64)
        return C.walk_wide(items, n, b, col, val, x, xs, bias, coef, _y0(d), tags, dtype, mis=mis)
    if form == 'pieces':
        return C.walk_onepass(p.items, p.n_items, None, col, val, x, xs, bias, coef, _y0(d), dtype, split=p.split, mis=mis)
    items, n, b = p.onepass(d)
    return C.walk_onepass(items, n, b, col, val, x, xs, bias, coef, _y0(d), dtype, mis=mis)


WALKS = [('onepass', 8), ('onepass', 36), ('onepass', 132), ('wide', 64), ('pieces', 8)]


@pytest.mark.parametrize('form,d', WALKS)
def test_walkers_give_the_reference_bit_for_bit_on_integer_data(plans, form, d):
    cases = [('full', 'fwd', o) for o in range(4)] + [('subset', 'fwd', 2), ('range', 'fwd', 1), ('full', 'bwd', 2), ('subset', 'bwd', 3)]
    for name, direction, option in cases:
        rows = C.plan_rows(name)
        ref = C.reference('int', option, direction)[:, :d]
        for dtype in (torch.float64, torch.float32):
            y = _walk(plans[name, direction], form, 'int', option, direction, d, dtype)
            assert torch.equal(y[rows].double(), ref[rows]), (form, d, name, direction, option, dtype)
            rest = torch.ones(C.N, dtype=torch.bool)
            rest[rows] = False
            assert bool((y[rest] == 7.0).all())


@pytest.mark.parametrize('form,d,mis', [('onepass', 8, 'gt'), ('onepass', 8, 'shift'), ('onepass', 64, 'gt'), ('onepass', 8, 'share'),
                                        ('onepass', 132, 'share'), ('wide', 64, 'tag'), ('wide', 64, 'share')])
def test_one_mis_decode_is_seen(plans, form, d, mis):
    """j > b for j >= b, count fields read 8 bits apart, a group member that stops one chunk short, the row tag dropped: the
    integer data tells each from the reference - on the rows it concerns, and on no other."""
    for option in (0, 1):
        ref = C.reference('int', option, 'fwd')[:, :d]
        y = _walk(plans['full', 'fwd'], form, 'int', option, 'fwd', d, mis=mis)
        wrong = (y != ref).any(1).nonzero().flatten().tolist()
        assert wrong, (form, d, mis)
        if mis == 'share':
            assert wrong == sorted(C.BIG)                                    # the rows whose members walk more than one chunk
        elif mis == 'shift':
            assert C.RUN_START['16x4'] + 2 in wrong and C.RUN_START['1_62_1'] + 2 in wrong and C.RUN_START['32_32'] not in wrong
        else:
            assert all(int(C.DEG[r]) <= 64 for r in wrong)
            assert C.RUN_START['32_32'] in wrong or C.RUN_START['32_32'] + 1 in wrong


def test_integer_data_is_exact_in_fp32_in_any_order():
    d = 128
    for direction in ('fwd', 'bwd'):
        rowptr, col = C.graph()[direction]
        for name in (None, 'w'):
            val = C.edge_values('int', name, direction)
            x = C.data('int')['x'][:, :d]
            ref = C.aggregate(rowptr, col, val, x, torch.float64)
            order = torch.randperm(col.numel(), generator=torch.Generator().manual_seed(5))
            a, b = C.aggregate(rowptr, col, val, x, torch.float32), C.aggregate(rowptr, col, val, x, torch.float32, order=order)
            assert torch.equal(a.double(), ref) and torch.equal(b.double(), ref)
            assert float(C.aggregate(rowptr, col, None if val is None else val.abs(), x.abs(), torch.float64).max()) < 2.0 ** 17
    assert float((C.data('int')['x'] * 8).frac().abs().max()) == 0.0 and set(C.data('int')['val']['w'].tolist()) == {0.25, 0.5, 1.0, 2.0}


def test_fp32_restatements_stay_inside_the_bound(plans):
    """The bound is derived (spmm_cases): here the fp32 host restatements are held to it, and their largest ratio is printed."""
    worst = {}
    for form, d in WALKS:
        for name, direction, option in (('full', 'fwd', 0), ('full', 'fwd', 2), ('full', 'bwd', 1), ('subset', 'fwd', 3)):
            rows = C.plan_rows(name)
            y = _walk(plans[name, direction], form, 'float', option, direction, d, torch.float32)
            ratio = C.error_ratio(y[rows], C.reference('float', option, direction)[rows, :d], C.bound(option, direction)[rows, :d])
            worst[form, d] = max(worst.get((form, d), 0.0), ratio)
    for option in range(4):
        for direction in ('fwd', 'bwd'):
            col, val, x, xs, bias, coef = C.operands('float', option, direction, 128)
            y = C.aggregate(C.graph()[direction][0], col, val, x, torch.float32)
            y = (y + coef * xs if coef else y)
            y = y + bias if bias is not None else y
            ratio = C.error_ratio(y, C.reference('float', option, direction)[:, :128], C.bound(option, direction)[:, :128])
            worst['index_add_', 128] = max(worst.get(('index_add_', 128), 0.0), ratio)
    for key, ratio in worst.items():
        print(f'fp32 restatement {key[0]} d={key[1]}: largest |err| / (gamma_k S) = {ratio:.3f}')
        assert ratio <= 1.0, (key, ratio)
    # a row without an edge, self term or bias has S = 0 and must be exactly 0
    empty = (C.degrees('fwd') == 0).nonzero().flatten()
    assert float(C.scale(1, 'fwd')[empty].min()) > 0 and float(C.bound(0, 'fwd')[empty].min()) > 0


def test_visit_arithmetic():
    assert C.launch_shape(816) == (208, 104) and C.launch_shape(816, cap=8) == (8, 4) and C.launch_shape(40000) == (8192, 4096)
    v = C.visit_of_items(24, [0, 12, 12, 16, 16, 16, 20, 24, 24], cap=8)
    assert v.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2] + [0] * 12
    assert C.visit_of_items(20, None, cap=8).tolist() == [0, 0, 0] * 6 + [0, 0]
    assert C.max_rows(4) == 4 and C.max_rows(32) == 4 and C.max_rows(36) == 2 and C.max_rows(64) == 2 and C.max_rows(68) == 1
