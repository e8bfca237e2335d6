"""SplitPlan.onepass_wide: the work items of the wide 64-float aggregation (up to 16 consecutive light rows per item, hub rows
as 4-aligned group quadruples), on a small random CSR with crafted rows and on a row-subset plan.  No GPU."""
import pytest
import torch

from gnndelete_amd.graph import SplitPlan


def _rowptr():
    g = torch.Generator().manual_seed(7)
    n = 3001
    deg = torch.randint(0, 13, (n,), generator=g)
    deg[0], deg[n - 1] = 3, 2
    deg[50:70] = 0                       # a run of rows without in-edges
    deg[100:140] = 1                     # 40 one-edge rows: items of 16 + a remainder
    deg[200:217] = 2                     # 17 light rows
    deg[300:304] = 16                    # exactly 64 in-edges together ...
    deg[304] = 1                         # ... and the row after them
    deg[400] = 64                        # a single row of 64 in-edges
    deg[500], deg[501], deg[503] = 65, 129, 1000      # hub rows directly between light rows (one above 4 pieces)
    deg[1500] = 257
    deg[99] = deg[140] = deg[199] = deg[299] = deg[399] = 70      # hub rows in front of the crafted runs: each run opens an item
    deg[401] = 5
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(deg, 0)]).to(torch.int32)


def _check(rowptr, plan, rows):
    items, n_items, bounds, tags = plan.onepass_wide(64)
    rp = rowptr.tolist()
    assert n_items == items.shape[0] and n_items % 4 == 0
    assert bounds.shape[0] == 9 and bool((bounds % 4 == 0).all()) and int(bounds[0]) == 0 and int(bounds[8]) == n_items
    assert bool((bounds[1:] >= bounds[:-1]).all())
    assert tags.shape[0] == rp[-1]
    covered = torch.zeros(rp[-1], dtype=torch.long)
    in_items = []
    it = items.tolist()
    i = 0
    hubs = []
    while i < n_items:
        row, start, end, slot = it[i]
        if row < 0:
            assert it[i] == [-1, 0, 0, -1]                                    # padding
            i += 1
        elif slot == -2:                                                       # a hub row: a 4-aligned quadruple
            assert i % 4 == 0 and all(m[0] == row and m[3] == -2 for m in it[i:i + 4])
            assert rp[row + 1] - rp[row] > 64 and it[i][1] == rp[row] and max(m[2] for m in it[i:i + 4]) == rp[row + 1]
            for w in range(4):
                ms, me = it[i + w][1], it[i + w][2]
                assert ms <= me and (w == 0 or ms == it[i + w - 1][2])
                covered[ms:me] += 1
                assert bool((tags[ms:me] == 0).all())
            hubs.append(row)
            i += 4
        else:
            nr = -slot - 15
            assert 1 <= nr <= 16 and end - start <= 64
            assert start == rp[row] and end == rp[row + nr]                    # consecutive rows, adjacent in the CSR
            for q in range(nr):
                assert rp[row + q + 1] - rp[row + q] <= 64
                assert bool((tags[rp[row + q]:rp[row + q + 1]] == q).all())    # tag = row - first row of the item < rows
                in_items.append(row + q)
            covered[start:end] += 1
            i += 1
    want = torch.zeros_like(covered)
    for r in rows:
        want[rp[r]:rp[r + 1]] = 1
    assert torch.equal(covered, want)                                          # every edge of every planned row exactly once
    light = sorted(r for r in rows if rp[r + 1] - rp[r] <= 64)
    assert sorted(in_items) == light and sorted(hubs) == sorted(r for r in rows if rp[r + 1] - rp[r] > 64)
    assert bool((tags[want == 0] == 0).all())
    return items


def test_wide_plan_packs_consecutive_light_rows_and_aligns_hub_groups():
    rowptr = _rowptr()
    n = rowptr.numel() - 1
    plan = SplitPlan(rowptr)
    items = _check(rowptr, plan, list(range(n)))
    by_row = {r[0]: r for r in items.tolist() if r[0] >= 0 and r[3] <= -16}
    assert -by_row[100][3] - 15 == 16 and -by_row[116][3] - 15 == 16 and -by_row[132][3] - 15 == 8     # 40 = 16 + 16 + 8 rows
    assert -by_row[300][3] - 15 == 4 and by_row[300][2] - by_row[300][1] == 64 and 304 in by_row     # a full item, then the next row
    assert -by_row[400][3] - 15 == 1
    assert 502 in by_row and -by_row[502][3] - 15 == 1                                                 # a light row between two hubs
    # far fewer items than the two-row form, and the greedy rule is deterministic
    assert plan.onepass_wide(64)[1] < plan.onepass(64)[1] // 2
    again = SplitPlan(rowptr).onepass_wide(64)
    assert torch.equal(again[0], plan.onepass_wide(64)[0]) and torch.equal(again[3], plan.onepass_wide(64)[3])
    # `onepass` is what it was
    assert int((plan.onepass(64)[0][:, 3] <= -16).sum()) > 500


@pytest.mark.parametrize('max_rows', [8, 1])
def test_wide_plan_rows_per_item_limit(max_rows):
    rowptr = _rowptr()
    plan = SplitPlan(rowptr)
    items = plan.onepass_wide(64, max_rows=max_rows)[0]
    wide = items[(items[:, 0] >= 0) & (items[:, 3] <= -16)]
    assert int((-wide[:, 3] - 15).max()) == max_rows


def test_wide_plan_on_a_row_subset():
    rowptr = _rowptr()
    n = rowptr.numel() - 1
    g = torch.Generator().manual_seed(3)
    rows = torch.cat([torch.randperm(n, generator=g)[:1800], torch.tensor([0, n - 1, 500, 501, 503]), torch.arange(100, 140)]).unique()
    plan = SplitPlan(rowptr, rows=rows)
    _check(rowptr, plan, rows.tolist())


def test_wide_plan_of_no_rows():
    rowptr = _rowptr()
    plan = SplitPlan(rowptr, rows=torch.zeros(0, dtype=torch.long))
    items, n_items, bounds, tags = plan.onepass_wide(64)
    assert n_items == 0 and items.shape == (0, 4) and bool((bounds == 0).all()) and int(tags.abs().sum()) == 0
