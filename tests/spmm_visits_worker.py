"""Child process of tests/test_spmm_forms_gpu.py::test_later_visits_of_the_item_kernel, started with GD_SPMM_GRID_CAP=8 in its
environment (the item kernel's launch reads the cap once per process): 8 blocks, 4 waves per XCD, so every wave sweeps its range
in many visits - the descriptor rotation, the one-visit-ahead index prefetch and the group barriers run on second, third and
later visits.  Holds the full and the subset plan at d = 8, 36, 64, 128, 260, one-launch and two-launch, to the checks of
spmm_cases.hold (integer data bit for bit, float data under the bound) and prints SPMM_VISITS_OK."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

CAP = 8


def main():
    import spmm_cases as C
    from gnndelete_amd import ops
    assert os.environ.get('GD_SPMM_GRID_CAP') == str(CAP)
    for name in ('full', 'subset'):
        for direction in ('fwd', 'bwd'):
            plan = C.split_plan(name, direction, 'cuda')
            rowptr, col = C.dev_graph(direction)
            launch = lambda val, x, bias, coef, y, xs: ops._spmm_raw(rowptr, col, val, x, bias, coef, C.N, plan, out=y, x_self=xs, wide=False)
            for d in (8, 36, 64, 128, 260):
                # the restated launch arithmetic: every wave that has an item makes at least 3 visits, group quadruples on later ones
                items, n, bounds = plan.onepass(d)
                assert C.launch_shape(n, CAP) == (8, 4)
                for length, visits in C.visits_per_wave(n, bounds, CAP):
                    assert length == 0 or visits >= 3, (name, direction, d, length)
                visit = C.visit_of_items(n, bounds, CAP)
                groups = [int(visit[i]) for i, _, _ in C.group_rows(items, n)]
                if direction == 'fwd':
                    assert groups and sum(v >= 2 for v in groups) >= len(groups) // 2 and max(groups) >= 8, groups
                assert (plan.n_items + 7) // 8 >= 12 and C.launch_shape(plan.n_items, CAP) == (8, 4)       # the piece form: equal eighths
                os.environ.pop('GD_SPMM_TWO_LAUNCH', None)
                one = C.hold(launch, d, name, direction, tag='later visits')
                os.environ['GD_SPMM_TWO_LAUNCH'] = '1'
                two = C.hold(launch, d, name, direction, tag='later visits, two-launch')
                os.environ.pop('GD_SPMM_TWO_LAUNCH', None)
                print(f'later visits (grid cap {CAP}) {name} {direction} d={d}: bit-exact on integer data, largest |err| / (gamma_k S) '
                      f'one-launch {one:.3f} two-launch {two:.3f}, up to {int(visit.max()) + 1} visits per wave', flush=True)
    torch.cuda.synchronize()
    print('SPMM_VISITS_OK')


if __name__ == '__main__':
    main()
