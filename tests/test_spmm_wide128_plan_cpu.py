"""The wide 128-float aggregation off the GPU: ops.spmm_wide128_form (which shapes _spmm_raw routes to
gd_spmm_csr_onepass_wide128_f32, at the edges of the 24-bit addressing conditions and under the A/B switches) and
SplitPlan.onepass_wide128 (the 64-float form's items and row tags, range limits at multiples of 4), walked on the host at 128
floats over the crafted CSR of spmm_cases.py: integer data gives the fp64 reference bit for bit under every plan."""
import torch

import spmm_cases as C
from gnndelete_amd import graph, ops


def test_predicate_and_its_bounds():
    n = 235868
    f = ops.spmm_wide128_form
    assert f(128, n, 128, 128, env={}) and f(128, n, 144, 132, env={})
    assert not f(64, n, 64, 64, env={}) and not f(132, n, 132, 132, env={}) and not f(256, n, 256, 256, env={})
    assert not ops.spmm_wide_form(128, n, 128, 128, env={})                     # the 64-float predicate stays what it was
    assert not f(128, n, 130, 128, env={})                                      # rows that are not 16-byte aligned
    # row ids below 2^24, pitches below 2^24 bytes, x and y below 4 GiB
    assert not f(128, 1 << 24, 128, 128, env={})                                # (at 512-byte rows the 4 GiB bound is the nearer one)
    assert f(128, 255, (1 << 22) - 4, 128, env={}) and not f(128, 255, 1 << 22, 128, env={}) and not f(128, 255, 128, 1 << 22, env={})
    assert f(128, (1 << 23) - 1, 128, 128, env={}) and not f(128, 1 << 23, 128, 128, env={})          # 2^23 rows x 512 B = 4 GiB
    assert not f(128, 1 << 22, 256, 128, env={}) and not f(128, 1 << 22, 128, 256, env={})
    # the switches
    assert not f(128, n, 128, 128, env={'GD_SPMM_D128_FORM': 'items'}) and f(128, n, 128, 128, env={'GD_SPMM_D128_FORM': 'wide'})
    assert not f(128, n, 128, 128, env={'GD_SPMM_TWO_LAUNCH': '1'}) and not f(128, n, 128, 128, env={'GD_SPMM_MULTIROW': '0'})
    assert f(128, n, 128, 128, env={'GD_SPMM_D64_FORM': 'pairs'})               # (the 64-float switch is the other form's)


def test_plan_reuses_the_items_and_tags_of_the_64_float_form():
    for name in C.PLANS:
        for direction in ('fwd', 'bwd'):
            plan = C.split_plan(name, direction)
            before = plan.onepass_wide(64)
            snap = [t.clone() if torch.is_tensor(t) else t for t in before]
            items, n, bounds, tags = plan.onepass_wide128()
            assert tags is before[3] and n % 4 == 0 and bool((bounds % 4 == 0).all()) and int(bounds[0]) == 0 and int(bounds[8]) == n
            if graph.WIDE128_VISIT_COST == graph.WIDE_VISIT_COST:
                assert items is before[0] and bounds is before[2]
            other = plan.onepass_wide128(visit_cost=24)                          # another cost: its own table, the same tags
            assert other[3] is before[3] and other[1] % 4 == 0 and bool((other[2] % 4 == 0).all())
            again = plan.onepass_wide(64)
            assert all((a is b) for a, b in zip(again, before))
            assert all(torch.equal(a, b) if torch.is_tensor(a) else a == b for a, b in zip(again, snap))
            # every entry of the plan's rows is summed once, into its own row
            ent, rows = C.item_edges(items, n, 'wide', tags=tags)
            rp = C.graph()[direction][0].long()
            want = torch.cat([torch.arange(int(rp[r]), int(rp[r + 1])) for r in C.plan_rows(name).tolist()])
            order = torch.argsort(ent)
            assert torch.equal(ent[order], want) and torch.equal(rows[order], C.row_of_entry(direction)[want])


def test_host_walk_at_128_floats_is_exact_on_integer_data():
    for name, direction, option in (('full', 'fwd', 0), ('subset', 'fwd', 2), ('range', 'bwd', 3), ('full', 'bwd', 1)):
        plan = C.split_plan(name, direction)
        items, n, bounds, tags = plan.onepass_wide128()
        col, val, x, xs, bias, coef = C.operands('int', option, direction, 128)
        y0 = torch.full((C.N, 128), C.SENTINEL, dtype=torch.float64)
        y = C.walk_wide(items, n, bounds, col, val, x, xs, bias, coef, y0, tags)
        rows = C.plan_rows(name)
        assert torch.equal(y[rows], C.reference('int', option, direction)[rows, :128])
        outside = torch.ones(C.N, dtype=torch.bool)
        outside[rows] = False
        assert bool((y[outside] == C.SENTINEL).all())
