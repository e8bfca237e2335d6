"""The three forms of the R-GCN typed conv - gd_rgcn_wave_conv_f32, gd_rgcn_tile_conv_f32, gd_rgcn_conv_f32 - against fp64 on
the host, PER ELEMENT, on the one graph of rgcn_cases.py that drives their plans to their edges (checked on the host by
test_rgcn_cases_cpu.py): a 672- and a 256-step tile behind the tile kernel's 256-slot step ring, hubs in one slice tile and
in twenty, a hub in the last, partial tile whose real tile is left without a step, steps of 1 / 16 / 17 / 32 pieces, a tile
without an edge, an odd tile count for the wave kernel's XCD pairing.

  A  every form x width pair x graph / mirror x trans 0 / 1 x 4-block / dense weights, raw through ops.rgcn_typed_accumulate
  B  the tile form under GD_RGCN_HUB_STEPS unset / 8 / 1000000000, and the cached y_ext buffer across output widths
  C  restrict_bwd: the affected-rows view of the transposed side, wave and tile forms
  D  the wave kernel's switches (XCD blocks, depth, blocks per wave, relu_in): the bits of the default
  E  the refusals of the tile and wave entry points

error = max |got - ref64| / s over the rows of a class, s = the same expression in fp64 on absolute values; bound =
max(8 x the larger error of the two fp32 restatements on the host, 2^-22) per (width pair, direction, row class), taken over
both graphs and both weight layouts.  Rows without an edge keep the bits they were preloaded with, the three sentinel rows
behind y stay, a second launch gives the same bits.

Measured on an MI355X (pytest -s prints every figure; the host's fp32 figures move in the last digit with its thread
count).  A: the largest scaled error per form over both graphs and both weight layouts (wave: 4 blocks only); the fp32
restatement is the larger of pyg.rgcn_conv in fp32 and the tile plan walked in fp32 on the host; hub = rows 5 and 393,
ring = the rows of the 672- and the 256-step tiles:

    widths      trans class   wave      tile      node-major  fp32 restatement  bound
    128 -> 128  0     hub     3.35e-08  3.35e-08  3.35e-08    3.35e-08          2.68e-07
    128 -> 128  0     ring    3.47e-08  3.47e-08  3.80e-08    3.80e-08          3.04e-07
    128 -> 128  0     rest    5.40e-08  5.40e-08  4.95e-08    4.93e-08          3.94e-07
    128 -> 128  1     hub     5.29e-08  5.29e-08  7.66e-08    5.92e-08          4.74e-07
    128 -> 128  1     ring    6.60e-08  7.25e-08  7.81e-08    7.81e-08          6.25e-07
    128 -> 128  1     rest    1.40e-07  1.40e-07  1.40e-07    1.40e-07          1.12e-06
    128 -> 64   0     hub     2.53e-08  3.83e-08  2.37e-08    2.58e-08          2.38e-07
    128 -> 64   0     ring    3.34e-08  3.34e-08  2.81e-08    2.81e-08          2.38e-07
    128 -> 64   0     rest    4.49e-08  5.93e-08  5.40e-08    5.40e-08          4.32e-07
    128 -> 64   1     hub     6.78e-08  6.78e-08  1.08e-07    8.17e-08          6.54e-07
    128 -> 64   1     ring    8.87e-08  8.87e-08  8.59e-08    8.81e-08          7.04e-07
    128 -> 64   1     rest    1.94e-07  1.94e-07  1.94e-07    2.08e-07          1.66e-06
     64 -> 128  0     hub     3.73e-08  3.73e-08  3.73e-08    3.73e-08          2.98e-07
     64 -> 128  0     ring    4.65e-08  4.65e-08  4.57e-08    4.57e-08          3.65e-07
     64 -> 128  0     rest    6.04e-08  6.04e-08  6.29e-08    6.29e-08          5.03e-07
     64 -> 128  1     hub     4.15e-08  4.82e-08  1.09e-07    9.00e-08          7.20e-07
     64 -> 128  1     ring    6.87e-08  6.87e-08  8.47e-08    8.47e-08          6.78e-07
     64 -> 128  1     rest    1.34e-07  1.09e-07  1.16e-07    1.16e-07          9.26e-07
     64 -> 64   0     hub     3.12e-08  2.79e-08  3.12e-08    3.12e-08          2.49e-07
     64 -> 64   0     ring    2.92e-08  2.92e-08  3.69e-08    3.69e-08          2.95e-07
     64 -> 64   0     rest    6.10e-08  7.26e-08  6.72e-08    6.72e-08          5.37e-07
     64 -> 64   1     hub     7.11e-08  7.11e-08  1.21e-07    9.36e-08          7.48e-07
     64 -> 64   1     ring    8.75e-08  8.75e-08  1.01e-07    1.01e-07          8.05e-07
     64 -> 64   1     rest    1.45e-07  1.45e-07  1.56e-07    1.56e-07          1.25e-06

   All three forms sit at the fp32 restatement's own error, a fifth of the bound or less: the plan's mean weights are
   fp32(1 / |run|), an error every edge of a run shares, and it is most of what any fp32 form of this sum is off by (the
   host walk of the same plan with 1 / |run| in fp64 meets the reference at 1e-12).  No form is less accurate on the hub rows
   or the 672-step rows than elsewhere; no defect was found in rgcn_tile.hip, rgcn_wave.hip, rgcn.hip or the plans.
B: hub thresholds unset / 8 / 1000000000 at most 0.16 / 0.14 / 0.14 of the bound; y_ext reused across 128, 64, 128 outputs
   and other sources at most 0.23.  C: restrict_bwd, wave and tile, at most 0.06 of the bound on the rows in the mask.
Wall time of this file: 9 s (5 s of it the host references, computed once).
"""
import collections
import math

import pytest
import torch

import rgcn_cases as C

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
FORMS = {'wave': ('gd_rgcn_wave_conv_f32', {}), 'tile': ('gd_rgcn_tile_conv_f32', {'GD_RGCN_WAVE': '0'}),
         'node-major': ('gd_rgcn_conv_f32', {'GD_RGCN_NODE_MAJOR': '1'})}
ENTRIES = tuple(entry for entry, _ in FORMS.values())
SWITCHES = ('GD_RGCN_WAVE', 'GD_RGCN_NODE_MAJOR', 'GD_RGCN_HUB_STEPS', 'GD_RGCN_WAVE_XCD_BLOCKS', 'GD_RGCN_WAVE_DEPTH', 'GD_RGCN_WAVE_BPW',
            'GD_RGCN_SORT_PIECES')
_GRAPHS = {}


def _form(monkeypatch, form=None, **env):
    """Every switch of the typed conv unset, then the form's and the caller's."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for k, v in dict(FORMS[form][1] if form else {}, **env).items():
        monkeypatch.setenv(k, v)


def _typed(name, fresh=False):
    """The graph on the device (shared by the tests that launch under the default plan switches; its plans are built on
    first use and kept)."""
    from gnndelete_amd.graph import TypedNodeCSR
    if fresh or name not in _GRAPHS:
        ei, et = C.edges(name)
        tg = TypedNodeCSR(ei.cuda(), et.cuda(), C.N_NODES, C.N_REL)
        if fresh:
            return tg
        _GRAPHS[name] = tg
    return _GRAPHS[name]


def _count_entries(monkeypatch):
    """Counts the calls of the three library entries (as test_rgat_kernels_gpu._count_branches does for ops)."""
    from gnndelete_amd import _lib
    handle, calls = _lib.lib(), collections.Counter()

    class Counting:
        def __getattr__(self, name):
            fn = getattr(handle, name)
            if name not in ENTRIES:
                return fn

            def counted(*a):
                calls[name] += 1
                return fn(*a)
            return counted
    monkeypatch.setattr(_lib, 'lib', lambda: Counting())
    return calls


def _operands(d_in, d_out, nb, trans, x=None):
    """(source rows, weight, preloaded rows, buffer with three sentinel rows behind them) of one launch on the device."""
    c = C.case(d_in, d_out)
    src = (c['gy'] if trans else c['x']) if x is None else x
    base = c['dx0'] if trans else c['y0']
    buf = torch.full((C.N_NODES + 3, base.shape[1]), SENTINEL, device='cuda')
    buf[:C.N_NODES] = base.cuda()
    return src.cuda(), c[nb].cuda(), base, buf


def _launch(tg, d_in, d_out, nb, trans, x=None, **kw):
    from gnndelete_amd import ops
    src, w, base, buf = _operands(d_in, d_out, nb, trans, x)
    ops.rgcn_typed_accumulate(tg, src, w, nb, trans, buf[:C.N_NODES], **kw)
    torch.cuda.synchronize()
    assert bool((buf[C.N_NODES:] == SENTINEL).all()), 'a row behind y was written'
    return buf[:C.N_NODES].cpu(), base


def _report(tag, errs, d_in, d_out, trans):
    print(f'[{tag}] ' + '  '.join(f'{cls} {e:.2e} (fp32 restatement {C.worst_restatement(d_in, d_out, trans, cls):.2e}, bound '
                                  f'{C.bound(d_in, d_out, trans, cls):.2e})' for cls, e in errs.items()))


# ---------------------------------------------------------------------------------------------------------------------
# A. every form against fp64, per element
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', C.GRAPHS)
@pytest.mark.parametrize('form,nb', [('wave', 4), ('tile', 4), ('tile', 1), ('node-major', 4), ('node-major', 1)])
def test_typed_conv_forms_hold_fp64_per_element(form, nb, name, monkeypatch):
    _form(monkeypatch, form)
    tg = _typed(name)
    if form == 'tile':
        for trans in (0, 1):
            C.assert_plan_figures(tg.tile_plan(bool(trans)), name, trans, None)
    if form == 'wave':
        for trans in (0, 1):
            tup = tg.wave_plan(bool(trans))['tile_unit_ptr'].long().cpu()
            assert (tup[1:] - tup[:-1]).tolist() == C.WAVE_UNITS['in' if (name == 'graph') != bool(trans) else 'out']
    calls = _count_entries(monkeypatch)
    for d_in, d_out in C.WIDTHS:
        for trans in (0, 1):
            calls.clear()
            got, base = _launch(tg, d_in, d_out, nb, trans)
            again, _ = _launch(tg, d_in, d_out, nb, trans)
            assert dict(calls) == {FORMS[form][0]: 2}, calls
            tag = f'{form} {name} {d_in}->{d_out} blocks {nb} trans {trans}'
            errs = C.check_rows(got, base, name, d_in, d_out, nb, trans, tag)
            _report(tag, errs, d_in, d_out, trans)
            assert torch.equal(got, again), tag


# ---------------------------------------------------------------------------------------------------------------------
# B. hub thresholds on the tile form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hub_steps', C.HUB_STEPS)
def test_tile_conv_under_every_hub_threshold(hub_steps, monkeypatch):
    """The plan reads GD_RGCN_HUB_STEPS when it is built and is cached with the graph: a fresh graph per setting."""
    _form(monkeypatch, 'tile', **({} if hub_steps is None else {'GD_RGCN_HUB_STEPS': str(hub_steps)}))
    calls = _count_entries(monkeypatch)
    for name in C.GRAPHS:
        tg = _typed(name, fresh=True)
        for trans in (0, 1):
            C.assert_plan_figures(tg.tile_plan(bool(trans)), name, trans, hub_steps)
        for d_in, d_out, nb in ((128, 64, 4), (64, 128, 1)):
            for trans in (0, 1):
                got, base = _launch(tg, d_in, d_out, nb, trans)
                tag = f'tile hub_steps {hub_steps} {name} {d_in}->{d_out} blocks {nb} trans {trans}'
                _report(tag, C.check_rows(got, base, name, d_in, d_out, nb, trans, tag), d_in, d_out, trans)
    assert dict(calls) == {'gd_rgcn_tile_conv_f32': 8}, calls


@pytest.mark.parametrize('hub_steps', (None, 8))
def test_tile_conv_reuses_its_slice_buffer_across_calls_and_widths(hub_steps, monkeypatch):
    """One plan with hubs, launched at 128, 64 and again 128 outputs with other sources each time: the y_ext buffers are
    cached per output width with the plan - a stale or wrongly sized one shows in the hub rows."""
    _form(monkeypatch, 'tile', **({} if hub_steps is None else {'GD_RGCN_HUB_STEPS': str(hub_steps)}))
    tg = _typed('graph', fresh=True)
    plan = tg.tile_plan(False)
    C.assert_plan_figures(plan, 'graph', 0, hub_steps)
    assert plan['n_hubs'] > 0
    seen = set()
    for d_in, d_out in ((128, 128), (128, 64), (64, 128), (128, 128)):
        got, base = _launch(tg, d_in, d_out, 4, 0)
        seen.add(d_out)
        tag = f'tile y_ext reuse hub_steps {hub_steps} {d_in}->{d_out}'
        _report(tag, C.check_rows(got, base, 'graph', d_in, d_out, 4, 0, tag), d_in, d_out, 0)
        assert set(plan['_y_ext']) == seen and plan['_y_ext'][d_out].shape == (plan['n_slice_rows'], d_out)
    # the same widths with other sources: x flipped row-wise (fp32-exact), against its own fp64 reference and scale
    buf128 = plan['_y_ext'][128]
    x2 = C.case(128, 128)['x'].flip(0).contiguous()
    got, base = _launch(tg, 128, 128, 4, 0, x=x2)
    assert plan['_y_ext'][128] is buf128
    ref, s = C.reference_for('graph', 128, 128, 4, x2)
    for cls in C.ROW_CLASSES:
        rows = C.class_rows('graph', 0, cls)
        err = float(((got.double()[rows] - ref[rows]).abs() / s[rows]).max())
        print(f'[tile y_ext reuse hub_steps {hub_steps} flipped x] {cls} {err:.2e}')
        assert err <= C.bound(128, 128, 0, cls), (cls, err)
    untouched = ~C.touched_rows('graph', 0)
    assert torch.equal(got[untouched], base[untouched])


# ---------------------------------------------------------------------------------------------------------------------
# C. restrict_bwd
# ---------------------------------------------------------------------------------------------------------------------
def _restrict_mask():
    """Keeps node 5, drops node 393, cuts through the 672- and the 256-step tiles, half of the rest."""
    mask = torch.rand(C.N_NODES, generator=torch.Generator().manual_seed(393)) < 0.5
    mask[[5, 64, 66, 68, 128, 130]] = True
    mask[[393, 65, 67, 69, 129, 131]] = False
    return mask


@pytest.mark.parametrize('form', ['wave', 'tile'])
def test_restricted_transposed_conv_touches_the_masked_rows_only(form, monkeypatch):
    """The mirror graph, whose hubs and long tiles sit on the transposed side: rows in the mask meet the bound against the
    UNRESTRICTED fp64 gradient, rows outside keep the preloaded bits."""
    _form(monkeypatch, form)
    mask = _restrict_mask()
    view = _typed('mirror').restrict_bwd(mask.cuda())
    if form == 'tile':
        fig = C.plan_figures(view.tile_plan(True))
        steps = fig['steps_per_tile']
        assert fig['hub_nodes'] == [5] and 256 < steps[1] < 672 and 64 < steps[2] < 256 and steps[6] == 0, fig
    calls = _count_entries(monkeypatch)
    for d_in, d_out in C.WIDTHS:
        got, base = _launch(view, d_in, d_out, 4, 1)
        again, _ = _launch(view, d_in, d_out, 4, 1)
        tag = f'{form} restrict_bwd {d_in}->{d_out}'
        _report(tag, C.check_rows(got, base, 'mirror', d_in, d_out, 4, 1, tag, rows_mask=mask), d_in, d_out, 1)
        assert torch.equal(got, again) and torch.equal(got[~mask], base[~mask])
    assert dict(calls) == {FORMS[form][0]: 8}, calls
    # the forward side of the view is the graph's own
    assert view.fwd is _typed('mirror').fwd


# ---------------------------------------------------------------------------------------------------------------------
# D. the wave kernel's switches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', C.GRAPHS)
def test_wave_conv_switches_give_the_bits_of_the_default(name, monkeypatch):
    """7 tiles: an odd count for the XCD pairing (the last pair holds one tile), 4 waves of a last group without a tile."""
    from gnndelete_amd import ops
    _form(monkeypatch, 'wave')
    tg = _typed(name)
    calls = _count_entries(monkeypatch)
    n_launch = 0
    for d_in, d_out in C.WIDTHS:
        for trans in (0, 1):
            _form(monkeypatch, 'wave')
            want, _ = _launch(tg, d_in, d_out, 4, trans)
            settings = [{'GD_RGCN_WAVE_XCD_BLOCKS': xb, 'GD_RGCN_WAVE_DEPTH': dp} for xb in '01' for dp in '13']
            if (d_out if trans else d_in) == 64:
                settings += [{'GD_RGCN_WAVE_BPW': '2'}, {'GD_RGCN_WAVE_BPW': '2', 'GD_RGCN_WAVE_DEPTH': '1'}]
            for env in settings:
                _form(monkeypatch, 'wave', **env)
                got, _ = _launch(tg, d_in, d_out, 4, trans)
                assert torch.equal(got, want), (d_in, d_out, trans, env)
            n_launch += 1 + len(settings)
    assert dict(calls) == {'gd_rgcn_wave_conv_f32': n_launch}, calls
    # relu_in: the conv of relu(x), formed where the gathered rows land = the conv of a clamped copy
    _form(monkeypatch, 'wave')
    for d_in, d_out in C.WIDTHS:
        for env in ({}, {'GD_RGCN_WAVE_XCD_BLOCKS': '1' if d_in == 64 else '0'}):
            _form(monkeypatch, 'wave', **env)
            src, w, base, buf = _operands(d_in, d_out, 4, 0)
            assert ops.rgcn_wave_relu_ok(tg, src, buf[:C.N_NODES], 4)
            got, _ = _launch(tg, d_in, d_out, 4, 0, relu_in=True)
            want, _ = _launch(tg, d_in, d_out, 4, 0, x=C.case(d_in, d_out)['x'].clamp(min=0))
            assert torch.equal(got, want), (d_in, d_out, env)


# ---------------------------------------------------------------------------------------------------------------------
# E. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_what_they_cannot_run(monkeypatch):
    """Argument checks that return an error code before any launch and leave y alone."""
    from gnndelete_amd import _lib, ops
    from gnndelete_amd._lib import ptr
    _form(monkeypatch, 'tile')
    lib = _lib.lib()
    tg = _typed('graph')
    n, d = C.N_NODES, 128
    p, wp = tg.tile_plan(False), tg.wave_plan(False)
    C.assert_plan_figures(p, 'graph', 0, None)
    n_real = math.ceil(n / 64)
    assert p['n_tiles'] == n_real + 1 and wp['n_tiles'] == n_real
    src, w, base, buf = _operands(d, d, 4, 0)
    xw = torch.zeros(n, 132, device='cuda')                          # rows at a pitch of 130 floats fit
    y = buf[:n]
    y_ext = torch.zeros(p['n_slice_rows'] + 4, d, device='cuda')
    packed = ops.rgcn_packed_weight(w, 4, d, d, 0)
    stream = _lib.stream_ptr(src.device)
    before = buf.clone()

    def tile(n_tiles=p['n_tiles'], x=src, ldx=d, d_in=d, out=y, hubs=True, ext=y_ext, n_blocks=4):
        return lib.gd_rgcn_tile_conv_f32(ptr(p['tile_order']), ptr(p['tile_step_ptr']), ptr(p['step_rel']), ptr(p['step_piece_ptr']),
                                         ptr(p['piece']), ptr(p['col']), ptr(p['w']), n_tiles, ptr(x), ldx, d_in, ptr(packed), n_blocks, 0,
                                         ptr(out), d, d, n, ptr(p['hub_node']) if hubs else None, ptr(p['hub_ptr']) if hubs else None,
                                         p['n_hubs'] if hubs else 0, ext if isinstance(ext, int) or ext is None else ptr(ext), stream)

    def wave(n_tiles=wp['n_tiles'], tile_size=64, x=src, out=y, n_blocks=4):
        return lib.gd_rgcn_wave_conv_f32(ptr(wp['job_tile']), n_tiles, tile_size, ptr(wp['tile_unit_ptr']), wp['n_units'], ptr(wp['unit_rel']),
                                         ptr(wp['unit_edges']), ptr(wp['unit_row']), ptr(x), d, d, ptr(packed), n_blocks, ptr(out), d, d, n, 0,
                                         stream)
    refused = {
        'tile: slice tiles without hub arrays': tile(hubs=False, ext=None),
        'tile: slice tiles without y_ext': tile(ext=None),
        'tile: n_tiles below ceil(n / 64)': tile(n_tiles=n_real - 1),
        'tile: a pitch that is no multiple of 4': tile(x=xw, ldx=130),
        'tile: a pitch below the width': tile(ldx=d - 4),
        'tile: x == y': tile(x=y),
        'tile: unaligned y_ext': tile(ext=y_ext.data_ptr() + 4),
        'tile: a width outside {64, 128}': tile(d_in=96),
        'tile: two diagonal blocks': tile(n_blocks=2),
        'wave: tile = 32': wave(tile_size=32),
        'wave: n_tiles one short': wave(n_tiles=n_real - 1),
        'wave: n_tiles one over': wave(n_tiles=n_real + 1),
        'wave: dense weights': wave(n_blocks=1),
        'wave: x == y': wave(x=y),
    }
    torch.cuda.synchronize()
    for what, rc in refused.items():
        assert rc != 0, what
    assert lib.gd_last_error_string().decode().startswith('gd_rgcn_wave_conv_f32')
    assert torch.equal(buf, before) and float(y_ext.abs().max()) == 0.0
    # and the same arguments unchanged run
    assert tile() == 0 and wave() == 0
    torch.cuda.synchronize()
    assert not torch.equal(buf, before) and bool((buf[n:] == SENTINEL).all())
