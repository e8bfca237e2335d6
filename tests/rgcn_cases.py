"""Shared inputs and references of the R-GCN typed-conv tests (test_rgcn_cases_cpu.py, test_rgcn_kernels_gpu.py): ONE
knowledge graph built for the edges of the plans TypedNodeCSR hands to gd_rgcn_tile_conv_f32 / gd_rgcn_wave_conv_f32 - a
tile of 672 steps and one of exactly 256 (the tile kernel's 256-slot step ring: first refill, wrap, a multiple of 64), two
hubs (one in the last, partial tile, whose real tile is left without a step), steps of 1 / 16 / 17 / 32 pieces, pieces of
8 / 9 / 16 edges, a tile without any edge - and its mirror (edge_index.flip(0)), on which the TRANSPOSED launch walks the
same structure.  Everything is deterministic from seeds and fp32-representable: drawn in fp32 and only then widened, so the
fp64 reference and the kernels read the same numbers.  References are computed once per process (lru_cache) and must be
left unchanged by their users.

    y  = y0  + sum_r mean_{e in run(i, r)} x[col_e] @ W_r            (trans = 0)
    dx = dx0 + d/dx sum(conv(x) * gy)                                 (trans = 1: the transposed graph with W_r^T)

The error of a result is per ELEMENT: max |got - ref64| / s over a set of rows, s = the same expression in fp64 on |x|,
|W|, |y0| (what the rounding of any summation order is relative to).  The bound of the GPU tests is
max(FACTOR x the larger scaled error of two fp32 restatements on the host, FLOOR) per (width pair, direction, row class):
pyg.rgcn_conv in fp32 and walk_tile_plan in fp32 (the tile kernel's order of additions) - never a kernel's output."""
import functools

import torch

from oracle import pyg_semantics as pyg
from rgat_cases import SOFTMAX_FACTOR as FACTOR, SOFTMAX_FLOOR as FLOOR

# ---------------------------------------------------------------------------------------------------------------------
# 1. the graph
# ---------------------------------------------------------------------------------------------------------------------
N_NODES, N_REL, TILE = 394, 100, 64                # six full tiles and a last tile of 10; relations 96..99 never occur
HUBS = (5, 393)                                    # 2,100 in-edges of relation 3 | 60 relations x 40 in-edges (last node)
RING_ROWS = tuple(range(64, 70))                   # tile 1: 16 relations x 101 in-edges each -> 96 relations x 7 passes
EXACT_ROWS = tuple(range(128, 132))                # tile 2: 16 relations x 64 in-edges each -> 64 relations x 4 passes
ISOLATED = (320, 384)                              # tile 5: no edge in or out
PIECE_RUNS = (8, 9, 15, 16, 17, 31, 32, 33)        # tile 4: runs on relations 60 .. 67 into the nodes 300 .. 307
SELF_LOOPS = ((5, 3), (64, 0), (393, 0), (200, 7))  # (node, relation)
GRAPHS = ('graph', 'mirror')
HUB_STEPS = (None, 8, 10 ** 9)                     # GD_RGCN_HUB_STEPS: the default (128), nearly every node a hub, no hub
WIDTHS = ((128, 128), (128, 64), (64, 128), (64, 64))
WEIGHTS = (4, 1)                                   # diagonal blocks: the reference's 4, dense
ROW_CLASSES = ('hub', 'ring', 'rest')


@functools.lru_cache(maxsize=None)
def plan_graph():
    """-> (edge_index [2, E], edge_type [E]).  Sources come from every node outside tile 5."""
    g = torch.Generator().manual_seed(39464)
    pool = torch.cat([torch.arange(0, ISOLATED[0]), torch.arange(ISOLATED[1], N_NODES)])
    src = lambda m: pool[torch.randint(0, pool.numel(), (m,), generator=g)]
    parts = []                                              # (sources, targets, relations)

    def add(s, d, r):                                       # d: one target or one per edge
        parts.append((s, torch.as_tensor(d).expand(s.numel()), torch.full((s.numel(),), r)))
    for k, node in enumerate(RING_ROWS):                    # 7 pieces per run, 112 piece-steps per node: no hub
        for r in range(16 * k, 16 * k + 16):
            add(src(101), node, r)
    for k, node in enumerate(EXACT_ROWS):                   # 4 full pieces per run
        for r in range(16 * k, 16 * k + 16):
            add(src(64), node, r)
    add(src(2100), HUBS[0], 3)                              # 132 pieces of one relation
    for r in range(60):
        add(src(40), HUBS[1], r)                            # 180 pieces
    add(src(33), torch.arange(192, 225), 50)                # tile 3: 33 one-edge runs of a relation = steps of 32 + 1 pieces
    add(src(17), torch.arange(192, 209), 51)                # 17 pieces: the second wave group works
    add(src(16), torch.arange(192, 208), 52)                # 16 pieces: it does not
    for i, m in enumerate(PIECE_RUNS):
        add(src(m), 300 + i, 60 + i)
    bg_pool = torch.cat([torch.arange(0, 64), torch.arange(192, 300)])
    bg = (src(3000), bg_pool[torch.randint(0, bg_pool.numel(), (3000,), generator=g)], torch.randint(0, 50, (3000,), generator=g))
    parts.append(bg)
    parts.append(tuple(t[:100] for t in bg))                # multi-edges of one relation
    loops = torch.tensor(SELF_LOOPS)
    parts.append((loops[:, 0], loops[:, 0], loops[:, 1]))
    ei = torch.stack([torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])])
    return ei.contiguous(), torch.cat([p[2] for p in parts]).contiguous()


def edges(name):
    ei, et = plan_graph()
    assert name in GRAPHS
    return (ei, et) if name == 'graph' else (ei.flip(0).contiguous(), et)


@functools.lru_cache(maxsize=None)
def typed_graph(name):
    """The TypedNodeCSR of a graph on the host (layout only; its plans are built with sorts / uniques in PyTorch)."""
    from gnndelete_amd.graph import TypedNodeCSR
    ei, et = edges(name)
    return TypedNodeCSR(ei, et, N_NODES, N_REL)


@functools.lru_cache(maxsize=None)
def tile_plan(name, trans, hub_steps=None, max_pieces=32):
    from gnndelete_amd.graph import TypedNodeCSR
    tg = typed_graph(name)
    return TypedNodeCSR._build_tile_plan(tg.bwd if trans else tg.fwd, N_NODES, N_REL, hub_steps=128 if hub_steps is None else hub_steps,
                                         max_pieces=max_pieces)


@functools.lru_cache(maxsize=None)
def wave_plan(name, trans):
    return typed_graph(name).wave_plan(bool(trans))


def plan_figures(p):
    """What the tests assert of a tile plan before they launch on it."""
    n_real = (N_NODES + TILE - 1) // TILE
    tsp, hp, hub = p['tile_step_ptr'].long().cpu(), p['hub_ptr'].tolist(), p['hub_node'].tolist()
    v = [b - a for a, b in zip(hp[:-1], hp[1:])] if p['n_hubs'] else []
    straddle = [hub[h] for h in range(p['n_hubs']) if hp[h] // TILE != (hp[h + 1] - 1) // TILE]
    return dict(n_hubs=p['n_hubs'], slice_sizes=sorted(set(v)), n_slice_rows=p['n_slice_rows'], n_tiles=p['n_tiles'],
                slice_tiles=p['n_tiles'] - n_real, steps_per_tile=(tsp[1:] - tsp[:-1]).tolist(), straddling=straddle,
                hub_nodes=hub[:p['n_hubs']] if p['n_hubs'] <= 4 else None)


# The figures of this graph's tile plans, (graph, trans, hub_steps) -> (hubs, slice sizes, slice rows, steps per REAL tile);
# the mirror's transposed side has the structure of the graph's forward side and the other way round.  The host asserts
# them of the plans it builds (test_rgcn_cases_cpu.py), the GPU tests of the plans built on the device.
def expected_figures(name, trans, hub_steps):
    return PLAN_FIGURES[('in' if (name == 'graph') != bool(trans) else 'out', hub_steps)]


_OUT = dict(n_hubs=0, hub_nodes=[], slice_sizes=[], n_slice_rows=0, straddles=False, steps=[138, 135, 134, 141, 143, 0, 94])
PLAN_FIGURES = {
    # 'in': the side on which the built rows are TARGETS (graph forward, mirror transposed); steps = per REAL tile
    ('in', None): dict(n_hubs=2, hub_nodes=[5, 393], slice_sizes=[4], n_slice_rows=64, straddles=False, steps=[50, 672, 256, 54, 63, 0, 0],
                       slice_steps=[92]),
    ('in', 8): dict(n_hubs=179, hub_nodes=None, slice_sizes=[4, 8, 16, 32, 64], n_slice_rows=1280, straddles=True,
                    steps=[13, 0, 0, 14, 13, 0, 0]),
    ('in', 10 ** 9): dict(n_hubs=0, hub_nodes=[], slice_sizes=[], n_slice_rows=0, straddles=False, steps=[181, 672, 256, 54, 63, 0, 180]),
    ('out', None): _OUT,
    ('out', 8): dict(n_hubs=330, hub_nodes=None, slice_sizes=[8, 16], n_slice_rows=5248, straddles=True, steps=[0] * 7),
    ('out', 10 ** 9): _OUT,
}
WAVE_UNITS = {'in': [122, 192, 64, 94, 64, 0, 60], 'out': [231, 226, 223, 228, 227, 0, 95]}


def assert_plan_figures(p, name, trans, hub_steps):
    """The plan `p` (built anywhere) has the figures this graph is known by."""
    want, got = expected_figures(name, trans, hub_steps), plan_figures(p)
    n_real = (N_NODES + TILE - 1) // TILE
    assert got['n_hubs'] == want['n_hubs'] and got['slice_sizes'] == want['slice_sizes'] and got['n_slice_rows'] == want['n_slice_rows'], got
    assert got['steps_per_tile'][:n_real] == want['steps'] and bool(got['straddling']) == want['straddles'], got
    assert got['slice_tiles'] == want['n_slice_rows'] // TILE and got['n_tiles'] == n_real + got['slice_tiles'], got
    if want['hub_nodes'] is not None:
        assert got['hub_nodes'] == want['hub_nodes'], got
    if 'slice_steps' in want:
        assert got['steps_per_tile'][n_real:] == want['slice_steps'], got


# ---------------------------------------------------------------------------------------------------------------------
# 2. inputs
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(d_in, d_out):
    """fp32 inputs of one width pair: x, the upstream gradient gy, the rows y0 / dx0 the launches add onto (in place of the
    root term), and the relation weights with 4 diagonal blocks and dense (scaled to the same output size)."""
    g = torch.Generator().manual_seed(1000 * d_in + d_out)
    return {'x': torch.randn(N_NODES, d_in, generator=g), 'gy': torch.randn(N_NODES, d_out, generator=g),
            'y0': torch.randn(N_NODES, d_out, generator=g), 'dx0': torch.randn(N_NODES, d_in, generator=g),
            4: torch.randn(N_REL, 4, d_in // 4, d_out // 4, generator=g) * 0.2,
            1: torch.randn(N_REL, d_in, d_out, generator=g) * 0.1}


def _conv(name, d_in, d_out, nb, dtype, absolute=False, x=None):
    """{'y', 'dx'} of pyg.rgcn_conv (root term replaced by y0) and its autograd input gradient (+ dx0) in `dtype`."""
    c = case(d_in, d_out)
    ei, et = edges(name)
    f = (lambda t: t.abs().to(dtype)) if absolute else (lambda t: t.to(dtype))
    xs = f(c['x'] if x is None else x).clone().requires_grad_()
    agg = pyg.rgcn_conv(xs, ei, et, f(c[nb]), torch.zeros(d_in, d_out, dtype=dtype), None, 4 if nb == 4 else None)
    agg.backward(f(c['gy']))
    return {'y': f(c['y0']) + agg.detach(), 'dx': f(c['dx0']) + xs.grad}


@functools.lru_cache(maxsize=None)
def reference_fp64(name, d_in, d_out, nb):
    return _conv(name, d_in, d_out, nb, torch.float64)


@functools.lru_cache(maxsize=None)
def scale_fp64(name, d_in, d_out, nb):
    """The per-element scale s: the same expressions on |x|, |W|, |gy|, |y0|, |dx0| (positive everywhere: |y0| > 0)."""
    return _conv(name, d_in, d_out, nb, torch.float64, absolute=True)


def reference_for(name, d_in, d_out, nb, x):
    """(y, s) in fp64 for another fp32 x of the same shape (not cached)."""
    return _conv(name, d_in, d_out, nb, torch.float64, x=x)['y'], _conv(name, d_in, d_out, nb, torch.float64, True, x=x)['y']


@functools.lru_cache(maxsize=None)
def touched_rows(name, trans):
    """bool [N]: the rows a launch adds to - nodes with an in-edge (trans: an out-edge).  Every other row keeps its bits."""
    ei, _ = edges(name)
    return torch.bincount(ei[0 if trans else 1], minlength=N_NODES) > 0


@functools.lru_cache(maxsize=None)
def class_rows(name, trans, cls):
    """Rows by class, among the touched ones: the two hub nodes, the nodes of the 672- and 256-step tiles, the rest.  (By node
    id in both directions: on the side where these nodes are sources they are ordinary rows.)"""
    ids = torch.arange(N_NODES)
    special = {'hub': HUBS, 'ring': RING_ROWS + EXACT_ROWS}
    if cls == 'rest':
        m = torch.ones(N_NODES, dtype=torch.bool)
        m[list(HUBS + RING_ROWS + EXACT_ROWS)] = False
    else:
        m = torch.zeros(N_NODES, dtype=torch.bool)
        m[list(special[cls])] = True
    return ids[m & touched_rows(name, trans)]


def scaled_error(got, name, d_in, d_out, nb, trans, rows=None):
    """max |got - ref64| / s over `rows` (default: every touched row) of y (trans: dx)."""
    key = 'dx' if trans else 'y'
    ref, s = reference_fp64(name, d_in, d_out, nb)[key], scale_fp64(name, d_in, d_out, nb)[key]
    rows = touched_rows(name, trans).nonzero().flatten() if rows is None else rows
    if rows.numel() == 0:
        return 0.0
    return float(((got.double()[rows] - ref[rows]).abs() / s[rows]).max())


# ---------------------------------------------------------------------------------------------------------------------
# 3. the tile plan walked on the host
# ---------------------------------------------------------------------------------------------------------------------
class RingError(AssertionError):
    """A read of the step ring found a slot that does not hold the step it was read for."""


class _Ring:
    """step_rel / step_piece_ptr of one tile behind rgcn_tile_kernel's 256-slot LDS ring, filled on its schedule."""
    SLOTS = 256

    def __init__(self, s0, s1, spp, srel):
        self.s0, self.s1, self.spp, self.srel = s0, s1, spp, srel
        self.pp, self.rel = [(-1, 0)] * self.SLOTS, [(-1, 0)] * self.SLOTS       # (step the slot holds, value)

    def fill(self, first, count):
        for s in range(first, first + count):
            if s <= self.s1:
                self.pp[(s - self.s0) % self.SLOTS] = (s, self.spp[s])
                if s < self.s1:
                    self.rel[(s - self.s0) % self.SLOTS] = (s, self.srel[s])

    def _read(self, slots, s, what):
        held, value = slots[(s - self.s0) % self.SLOTS]
        if held != s:
            raise RingError(f'{what} of step {s - self.s0} of a {self.s1 - self.s0}-step tile read from a slot that holds step {held - self.s0}')
        return value

    def desc(self, s):                                      # load_desc(s): the step's piece range, fetched two steps ahead
        if s < self.s1:
            return self._read(self.pp, s, 'piece pointer'), self._read(self.pp, s + 1, 'piece pointer')
        return 0, 0

    def step(self, s):
        return self._read(self.pp, s, 'piece pointer'), self._read(self.pp, s + 1, 'piece pointer'), self._read(self.rel, s, 'relation')


def dense_weights(w, nb, trans):
    """[R, agg width, out width] of one direction: the block-diagonal matrix written out, transposed for trans."""
    if nb == 4:
        r, _, ib, ob = w.shape
        full = torch.zeros(r, 4 * ib, 4 * ob, dtype=w.dtype)
        for b in range(4):
            full[:, b * ib:(b + 1) * ib, b * ob:(b + 1) * ob] = w[:, b]
    else:
        full = w
    return full.transpose(1, 2).contiguous() if trans else full


def walk_tile_plan(p, x, wdir, y0, dtype, fixup=True, refill_ahead=128, piece_cap=32):
    """What gd_rgcn_tile_conv_f32 does with a plan of TypedNodeCSR._build_tile_plan, in `dtype` (fp32: its order of
    additions): per tile in tile_order, per step, per piece - the piece's edges weight-summed one by one into a compact row,
    the step's compact rows times the step's relation weight added into the tile's accumulator rows named by the piece words
    (at most `piece_cap` pieces of a step: the kernel's 8 waves take 4 each), the accumulators added to y, those of slice rows
    written to a y_ext image that the fix-up adds to the hub_node rows in slice order.  step_rel / step_piece_ptr are read
    through the 256-slot ring on the kernel's schedule (192 slots up front, 64 more at +`refill_ahead` after every 64th
    step); a read that finds another step's slot raises RingError."""
    n = N_NODES
    x, wdir, y = x.to(dtype), wdir.to(dtype), y0.to(dtype).clone()
    d_out = wdir.shape[2]
    n_pc = p['n_pieces']
    piece = p['piece'].long()[:n_pc]
    e0, prow, plen = piece[:, 0], piece[:, 1] & 255, piece[:, 1] >> 8
    col, w = p['col'].long(), p['w'].to(dtype)
    if dtype == torch.float64:                              # the plan carries fp32(1 / |run|); fp64 takes 1 / |run| itself
        w = 1.0 / torch.round(1.0 / w)
    a = torch.zeros(n_pc, x.shape[1], dtype=dtype)
    for k in range(16):                                     # edge k of every piece, in edge order
        m = (plen > k).nonzero().flatten()
        if m.numel():
            a[m] += w[e0[m] + k][:, None] * x[col[e0[m] + k]]
    n_real = (n + TILE - 1) // TILE
    n_pad = n_real * TILE
    y_ext = torch.zeros(max(p['n_slice_rows'], 1), d_out, dtype=dtype)
    tsp, spp, srel = p['tile_step_ptr'].tolist(), p['step_piece_ptr'].tolist(), p['step_rel'].tolist()
    for tile in p['tile_order'].tolist():
        s0, s1 = tsp[tile], tsp[tile + 1]
        if s0 == s1:
            continue
        acc = torch.zeros(TILE, d_out, dtype=dtype)
        ring = _Ring(s0, s1, spp, srel)
        ring.fill(s0, 192)
        for s in (s0, s0 + 1, s0 + 2):
            ring.desc(s)
        for s in range(s0, s1):
            p0, p1, rel = ring.step(s)
            assert (p0, p1, rel) == (spp[s], spp[s + 1], srel[s])
            cnt = min(p1 - p0, piece_cap)
            acc[prow[p0:p0 + cnt]] += a[p0:p0 + cnt] @ wdir[rel]
            ring.desc(s + 3)
            if (s + 1 - s0) % 64 == 0:
                ring.fill(s + 1 + refill_ahead, 64)
        lo = tile * TILE
        if lo < n:
            y[lo:min(lo + TILE, n)] += acc[:min(TILE, n - lo)]
        elif lo >= n_pad:
            y_ext[lo - n_pad:lo - n_pad + TILE] = acc
    if fixup and p['n_hubs']:
        hp, hub = p['hub_ptr'].long(), p['hub_node'].long()[:p['n_hubs']]
        v = hp[1:] - hp[:-1]
        tot = torch.zeros(p['n_hubs'], d_out, dtype=dtype)
        for k in range(int(v.max())):                       # slice k of every hub, in slice order
            m = (v > k).nonzero().flatten()
            tot[m] += y_ext[hp[:-1][m] + k]
        y[hub] += tot
    return y


def walk(name, d_in, d_out, nb, trans, dtype, hub_steps=None, **kw):
    """walk_tile_plan on a case: y (trans: dx) of the graph's tile plan of that direction."""
    c = case(d_in, d_out)
    p = kw.pop('plan', None) or tile_plan(name, bool(trans), hub_steps)
    return walk_tile_plan(p, c['gy'] if trans else c['x'], dense_weights(c[nb], nb, trans), c['dx0'] if trans else c['y0'], dtype, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the bound
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restatement_errors(name, d_in, d_out, nb, trans, cls):
    """(pyg.rgcn_conv in fp32, walk_tile_plan in fp32): scaled errors to fp64 over the rows of a class."""
    rows = class_rows(name, trans, cls)
    return (scaled_error(_fp32_conv(name, d_in, d_out, nb)['dx' if trans else 'y'], name, d_in, d_out, nb, trans, rows),
            scaled_error(_fp32_walk(name, d_in, d_out, nb, trans), name, d_in, d_out, nb, trans, rows))


@functools.lru_cache(maxsize=None)
def _fp32_conv(name, d_in, d_out, nb):
    return _conv(name, d_in, d_out, nb, torch.float32)


@functools.lru_cache(maxsize=None)
def _fp32_walk(name, d_in, d_out, nb, trans):
    return walk(name, d_in, d_out, nb, trans, torch.float32)


@functools.lru_cache(maxsize=None)
def worst_restatement(d_in, d_out, trans, cls):
    """The larger fp32 restatement error of a width pair, direction and row class, over both graphs and both weight layouts."""
    return max(max(restatement_errors(name, d_in, d_out, nb, trans, cls)) for name in GRAPHS for nb in WEIGHTS)


def bound(d_in, d_out, trans, cls):
    """max(FACTOR x worst_restatement, FLOOR = 2^-22).  From the references alone."""
    return max(FACTOR * worst_restatement(d_in, d_out, trans, cls), FLOOR)


def check_rows(got, y0, name, d_in, d_out, nb, trans, tag, rows_mask=None):
    """The assertions every launch is held to: per class within its bound (rows_mask: only those rows were to be touched),
    every other row the bits of y0.  -> {class: error} (printed by the caller)."""
    touched = touched_rows(name, trans) if rows_mask is None else touched_rows(name, trans) & rows_mask
    out = {}
    for cls in ROW_CLASSES:
        rows = class_rows(name, trans, cls)
        rows = rows[touched[rows]]
        out[cls] = scaled_error(got, name, d_in, d_out, nb, trans, rows)
    for cls, err in out.items():
        assert err <= bound(d_in, d_out, trans, cls), (tag, cls, err, bound(d_in, d_out, trans, cls))
    assert torch.equal(got[~touched], y0[~touched]), (tag, 'a row without an edge changed')
    return out
