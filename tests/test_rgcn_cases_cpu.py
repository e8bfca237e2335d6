"""The inputs of test_rgcn_kernels_gpu.py, checked without a GPU: that the graph of rgcn_cases.py drives the tile and wave
plans of TypedNodeCSR to the edges it is built for (a 672- and a 256-step tile behind the tile kernel's 256-slot ring, hubs
in one and in many slice tiles, steps of 1 / 16 / 17 / 32 pieces, ...), that the tile plan keeps what rgcn_tile_kernel relies
on, that walking it on the host the way the kernel does gives the fp64 reference - and stops doing so when the walk is
wrong -, and the errors of the two fp32 restatements the GPU bound is made of.  Every figure is printed (pytest -s)."""
import pytest
import torch

import rgcn_cases as C

N_REAL = (C.N_NODES + C.TILE - 1) // C.TILE
SIDES = [(name, trans) for name in C.GRAPHS for trans in (0, 1)]


def _step_sizes(p):
    spp = p['step_piece_ptr'].long()
    return spp[1:] - spp[:-1]


def test_plan_graph_has_the_edges_it_is_built_for():
    ei, et = C.plan_graph()
    n = C.N_NODES
    assert ei.shape == (2, 21623) and et.shape == (21623,) and int(ei.min()) >= 0 and int(ei.max()) == n - 1
    lo, hi = C.ISOLATED
    assert not bool(((ei >= lo) & (ei < hi)).any())                                   # tile 5: no edge in or out
    rel = torch.bincount(et, minlength=C.N_REL)
    assert int(rel[96:].sum()) == 0 and int(rel[:68].min()) > 0 and int(et.max()) < 96
    run = torch.bincount(ei[1] * C.N_REL + et, minlength=n * C.N_REL).view(n, C.N_REL)
    for k, node in enumerate(C.RING_ROWS):
        want = torch.zeros(C.N_REL, dtype=torch.long)
        want[16 * k:16 * k + 16] = 101
        want[0] += node == 64                                                           # the self loop
        assert torch.equal(run[node], want)
    for k, node in enumerate(C.EXACT_ROWS):
        want = torch.zeros(C.N_REL, dtype=torch.long)
        want[16 * k:16 * k + 16] = 64
        assert torch.equal(run[node], want)
    assert int(run[128:192].sum()) == 4 * 16 * 64                                      # nothing else targets tile 2
    assert int(run[64:128].sum()) == 6 * 16 * 101 + 1
    assert int(run[5, 3]) >= 2101 and -(-int(run[5, 3]) // 16) == 132
    assert torch.equal(run[393, :60], torch.tensor([41] + [40] * 59)) and int(run[393, 60:].sum()) == 0
    assert int(run[384:393].sum()) == 0                                                 # the last tile's only target is its hub
    assert int((run[192:256, 50] == 1).sum()) == 33 and int((run[192:256, 51] == 1).sum()) == 17 and int((run[192:256, 52] == 1).sum()) == 16
    assert int(run[192:256, 50:].sum()) == 66 and int(run[:64, 50:].sum()) == 0        # background relations are 0 .. 49
    assert [int(run[300 + i, 60 + i]) for i in range(8)] == list(C.PIECE_RUNS) and int(run[300:320].sum()) == sum(C.PIECE_RUNS)
    key = (et * n + ei[1]) * n + ei[0]
    assert ei.shape[1] - int(key.unique().numel()) >= 100                              # multi-edges of one relation
    loops = ei[0] == ei[1]
    assert {(int(a), int(b)) for a, b in zip(ei[0, loops], et[loops])} >= set(C.SELF_LOOPS)
    m_ei, m_et = C.edges('mirror')
    assert torch.equal(m_ei, ei.flip(0)) and torch.equal(m_et, et)
    for d_in, d_out in C.WIDTHS:
        c = C.case(d_in, d_out)
        assert all(v.dtype == torch.float32 for v in c.values())
        assert c['x'].shape == c['dx0'].shape == (n, d_in) and c['gy'].shape == c['y0'].shape == (n, d_out)
        assert c[4].shape == (C.N_REL, 4, d_in // 4, d_out // 4) and c[1].shape == (C.N_REL, d_in, d_out)
        assert float(c['y0'].abs().min()) > 0 and float(c['dx0'].abs().min()) > 0     # the scale is positive everywhere


@pytest.mark.parametrize('hub_steps', C.HUB_STEPS)
@pytest.mark.parametrize('name,trans', SIDES)
def test_tile_plan_has_its_figures_and_keeps_what_the_kernel_relies_on(name, trans, hub_steps):
    p = C.tile_plan(name, bool(trans), hub_steps)
    arrays = C.typed_graph(name).bwd if trans else C.typed_graph(name).fwd
    C.assert_plan_figures(p, name, trans, hub_steps)
    fig = C.plan_figures(p)
    print(f'[tile plan {name} trans {trans} hub_steps {hub_steps}] ' + '  '.join(f'{k} {v}' for k, v in fig.items() if k != 'straddling')
          + f'  straddling hubs {len(fig["straddling"])}')
    n_pc, n_steps, e = p['n_pieces'], p['n_steps'], int(arrays[3].numel())
    piece = p['piece'].long()[:n_pc]
    e0, prow, plen = piece[:, 0], piece[:, 1] & 255, piece[:, 1] >> 8
    sizes = _step_sizes(p)
    tsp = p['tile_step_ptr'].long()
    steps_per_tile = tsp[1:] - tsp[:-1]
    # every edge sits in exactly one piece; pieces hold 1 .. 16 edges, steps 1 .. 32 pieces
    assert int(plen.min()) >= 1 and int(plen.max()) <= 16 and int(plen.sum()) == e == 21623
    cover = torch.zeros(e + 1, dtype=torch.long)
    cover.index_add_(0, e0, torch.ones_like(e0))
    cover.index_add_(0, e0 + plen, -torch.ones_like(e0))
    assert bool((torch.cumsum(cover, 0)[:e] == 1).all())
    assert sizes.numel() == n_steps and int(sizes.min()) >= 1 and int(sizes.max()) <= 32 and int(sizes.sum()) == n_pc
    assert int(tsp[-1]) == n_steps and p['tile_step_ptr'].numel() == p['n_tiles'] + 1 and p['max_steps'] == int(steps_per_tile.max())
    assert sorted(p['tile_order'].tolist()) == list(range(p['n_tiles']))
    assert bool((steps_per_tile[p['tile_order'].long()][1:] <= steps_per_tile[p['tile_order'].long()][:-1]).all())      # heaviest first
    # the rows of a step are distinct (plain read-modify-write in the kernel); relations ascend inside a tile
    step_of_piece = torch.repeat_interleave(torch.arange(n_steps), sizes)
    assert int((step_of_piece * C.TILE + prow).unique().numel()) == n_pc and int(prow.max()) < C.TILE
    srel = p['step_rel'].long()[:n_steps]
    tile_of_step = torch.repeat_interleave(torch.arange(p['n_tiles']), steps_per_tile)
    same_tile = tile_of_step[1:] == tile_of_step[:-1]
    assert bool((srel[1:][same_tile] >= srel[:-1][same_tile]).all()) and int(srel.max()) < 96
    # real tiles hold node rows that are no hub, slice tiles the rows hub_ptr counts: slice rows sit at n_pad and beyond
    grow = tile_of_step[step_of_piece] * C.TILE + prow
    hubs = set(p['hub_node'][:p['n_hubs']].tolist())
    hp = p['hub_ptr'].long()
    real = grow < N_REAL * C.TILE
    assert all(g < C.N_NODES for g in grow[real].tolist()) and not (set(grow[real].tolist()) & hubs)
    assert bool((hp[1:] > hp[:-1]).all()) and int(hp[0]) == 0
    if p['n_hubs']:
        assert bool((grow[~real] - N_REAL * C.TILE < hp[-1]).all()) and p['n_slice_rows'] - C.TILE < int(hp[-1]) <= p['n_slice_rows']
        assert p['n_tiles'] > N_REAL
    else:
        assert bool(real.all()) and p['n_tiles'] == N_REAL and p['n_slice_rows'] == 0
    assert torch.equal(p['w'].sort().values, arrays[4].sort().values) and torch.equal(p['col'].sort().values, arrays[3].sort().values)
    side = 'in' if (name == 'graph') != bool(trans) else 'out'
    if side == 'in' and hub_steps is None:
        st = fig['steps_per_tile']
        assert max(st) >= 449 and st[1] == 672 and 256 in st and st[2] == 256      # beyond the second refill's slots | a full ring
        assert st[6] == 0 and 393 in hubs and st[5] == 0                            # an empty real tile beside its hub | the isolated tile
        assert st[N_REAL] > 0 and fig['slice_tiles'] == 1
        assert {1, 16, 17, 32} <= set(sizes.tolist())
        assert {8, 9, 16} <= set(plen.tolist()) and {1, 15} <= set(plen.tolist())
    if side == 'in' and hub_steps == 8:
        assert fig['slice_sizes'] == [4, 8, 16, 32, 64] and fig['slice_tiles'] > 1 and {5, 393} <= set(fig['straddling'])
        assert 0 in fig['steps_per_tile'][N_REAL:]                                  # a slice tile no piece went to
    if side == 'in' and hub_steps == 10 ** 9:
        assert fig['steps_per_tile'][0] >= 132 and fig['steps_per_tile'][6] == 180  # the hubs' runs, one pass after the other
    if side == 'out':
        assert fig['steps_per_tile'][5] == 0 and (hub_steps != 8 or fig['slice_tiles'] > 64)


@pytest.mark.parametrize('name,trans', SIDES)
def test_wave_plan_has_its_units(name, trans):
    p = C.wave_plan(name, trans)
    tup = p['tile_unit_ptr'].long()
    units = (tup[1:] - tup[:-1]).tolist()
    print(f'[wave plan {name} trans {trans}] units per tile {units}')
    assert units == C.WAVE_UNITS['in' if (name == 'graph') != bool(trans) else 'out']
    assert p['n_tiles'] == N_REAL == 7 and N_REAL % 2 == 1 and units[5] == 0      # an odd tile count for the XCD pairing | 0 units
    assert int((p['unit_edges'][..., 0] != C.N_NODES).sum()) == 21623


@pytest.mark.parametrize('nb', C.WEIGHTS)
@pytest.mark.parametrize('hub_steps', C.HUB_STEPS)
@pytest.mark.parametrize('name', C.GRAPHS)
def test_walking_the_tile_plan_in_fp64_gives_the_reference(name, hub_steps, nb):
    for d_in, d_out in ((128, 64), (64, 128)):
        for trans in (0, 1):
            got = C.walk(name, d_in, d_out, nb, trans, torch.float64, hub_steps)
            err = C.scaled_error(got, name, d_in, d_out, nb, trans)
            c = C.case(d_in, d_out)
            base = (c['dx0'] if trans else c['y0']).double()
            print(f'[fp64 walk {name} {d_in}->{d_out} blocks {nb} trans {trans} hub_steps {hub_steps}] {err:.2e}')
            assert err < 1e-12
            assert torch.equal(got[~C.touched_rows(name, trans)], base[~C.touched_rows(name, trans)])


def test_a_wrong_walk_misses_the_reference_or_trips_the_ring():
    """Sensitivity on the host (no altered kernel runs on a GPU: a wrong ring hands the kernel piece indices out of range)."""
    d_in, d_out, nb = 128, 64, 4
    err = lambda got, rows=None: C.scaled_error(got, 'graph', d_in, d_out, nb, 0, rows)
    hub_rows, rest = C.class_rows('graph', 0, 'hub'), C.class_rows('graph', 0, 'rest')
    # the fix-up dropped: the hub rows alone are wrong (here and with nearly every row a hub)
    got = C.walk('graph', d_in, d_out, nb, 0, torch.float64, fixup=False)
    assert err(got, hub_rows) > 0.1 and err(got, rest) < 1e-12
    assert err(C.walk('graph', d_in, d_out, nb, 0, torch.float64, 8, fixup=False), rest) > 0.1
    # steps of up to 64 pieces, of which a block's 8 waves x 4 take 32
    crowded = C.tile_plan('graph', False, None, max_pieces=64)
    assert int(_step_sizes(crowded).max()) == 33
    got = C.walk('graph', d_in, d_out, nb, 0, torch.float64, plan=crowded)
    assert err(got) > 1e-3 and err(got, hub_rows) < 1e-12
    # the ring on another schedule.  Refilled at + 192 or + 0 instead of + 128 the slots 192 .. 255 are not there when the 256-
    # and the 672-step tiles read them (at + 0 they arrive three steps late); tiles of up to 192 steps never read a refill
    for ahead in (192, 0, 10 ** 6):
        for hub_steps in (None, 10 ** 9):
            with pytest.raises(C.RingError):
                C.walk('graph', d_in, d_out, nb, 0, torch.float64, hub_steps, refill_ahead=ahead)
        got = C.walk('graph', d_in, d_out, nb, 1, torch.float64, refill_ahead=ahead)             # 143 steps at most
        assert C.scaled_error(got, 'graph', d_in, d_out, nb, 1) < 1e-12
    only_exact = dict(C.tile_plan('graph', False), tile_order=torch.tensor([2], dtype=torch.int32))
    only_ring = dict(only_exact, tile_order=torch.tensor([1], dtype=torch.int32))
    with pytest.raises(C.RingError, match='step 192 of a 256-step tile'):
        C.walk('graph', d_in, d_out, nb, 0, torch.float64, plan=only_exact, refill_ahead=192)
    with pytest.raises(C.RingError, match='step 192 of a 672-step tile'):
        C.walk('graph', d_in, d_out, nb, 0, torch.float64, plan=only_ring, refill_ahead=0)
    # 256 slots of which 192 are filled up front leave the refill a window: + 64 (the block that is read next) holds as well
    # as the kernel's + 128, and both walk the 672 steps and the piece pointer one past step 255 (slot 0 again)
    for ahead in (128, 64):
        for plan in (only_exact, only_ring):
            C.walk('graph', d_in, d_out, nb, 0, torch.float64, plan=plan, refill_ahead=ahead)


@pytest.mark.parametrize('d_in,d_out', C.WIDTHS)
def test_fp32_restatements_and_the_gpu_bound(d_in, d_out):
    """The GPU bound is max(8 x the larger restatement error, 2^-22) per (width pair, direction, row class): both restatements
    stay below the floor, so no bound exceeds 8 x 2^-22 = 1.9e-6 of the element's scale."""
    for trans in (0, 1):
        for cls in C.ROW_CLASSES:
            b = C.bound(d_in, d_out, trans, cls)
            for name in C.GRAPHS:
                assert C.class_rows(name, trans, cls).numel() > 0
                for nb in C.WEIGHTS:
                    e_pyg, e_walk = C.restatement_errors(name, d_in, d_out, nb, trans, cls)
                    print(f'[{d_in}->{d_out} trans {trans} {cls:4s} {name:6s} blocks {nb}] fp32 pyg.rgcn_conv {e_pyg:.2e}  fp32 walk {e_walk:.2e}  bound {b:.2e}')
                    assert max(e_pyg, e_walk) <= C.FLOOR and C.FACTOR * max(e_pyg, e_walk) <= b
            assert C.FLOOR <= b <= C.FACTOR * C.FLOOR
