"""The inputs of test_rgat_kernels_gpu.py, checked without a GPU: that they have the rows, degrees, relations and logit
spans they are built for, and that the fp32 oracle ALONE sits inside every bound the GPU tests hold the kernels to - so a
kernel that misses a bound is wrong, not merely fp32.  Every distance is printed (pytest -s)."""
import pytest
import torch

import rgat_cases as C
from helpers import rel_l2


def test_softmax_segments_have_the_rows_they_are_built_for():
    rowptr = C.softmax_rowptr()
    lens = (rowptr[1:] - rowptr[:-1]).tolist()
    assert lens == [0, 1, 63, 64, 65, 0, 128, 129, 1000, 5000, 2, 0] and rowptr.dtype == torch.int32
    assert lens[0] == 0 and lens[5] == 0 and lens[-1] == 0                           # empty rows first, inside and last
    trips = sorted({-(-l // 64) for l in lens if l})
    assert trips == [1, 2, 3, 16, 79] and 5000 % 64 != 0 and 1000 % 64 != 0         # 1, 2 and 79 trips, partial last trips
    assert [int(C.softmax_rowptr(p)[-1]) for p in C.PREFIXES] == [0, 128, 193, sum(lens)]
    assert set(C.PREFIXES) >= {1, 4, 5} and len(lens) % 4 == 0                       # one row, one full block, one row more
    up = C.softmax_upstream()
    for regime in C.REGIMES:
        e = C.softmax_logits(regime)
        assert e.dtype == torch.float32 and e.numel() == sum(lens) and bool(torch.isfinite(e).all())
    assert float(C.softmax_logits('randn').abs().max()) < 6
    wide = C.softmax_logits('wide')
    assert bool(torch.isinf(torch.exp(wide.max()))) and float(torch.exp(wide.min() - wide.max())) == 0.0
    assert float(C.softmax_logits('offset').min()) > 2.9e4
    assert bool((C.softmax_logits('equal') == 7.25).all())
    dom = C.softmax_logits('dominant')
    assert int((dom > 50).sum()) == len(range(0, sum(lens), 97)) and float(dom[1::97].max()) < 6
    assert up.dtype == torch.float32 and up.numel() == sum(lens)


@pytest.mark.parametrize('regime', C.REGIMES)
def test_fp32_softmax_restatement_is_inside_the_gpu_bound(regime):
    """The GPU bound is max(8 x the fp32 restatement's error, 2^-22) per element: the restatement itself stays below the
    floor, so the bound never exceeds 8 x 2^-22 = 1.9e-6 on values that are at most 1."""
    for n_rows in C.PREFIXES:
        a64, d64 = C.softmax_reference_fp64(regime, n_rows)
        assert bool(torch.isfinite(a64).all()) and bool(torch.isfinite(d64).all())
        ea, ed, es = C.softmax_restatement_errors(regime, n_rows)
        ba, bd = C.softmax_bounds(regime, n_rows)
        # the row sums: index_add adds a row's terms one by one, which drifts (2e-6 over the 5,000-entry row) - the bound on
        # them is held against fp32 with pairwise row sums, the order a kernel's lanes-then-wave reduction resembles
        rw = C.softmax_rowwise_fp32(regime, n_rows)
        ew, _, esw = C.softmax_errors(rw, torch.zeros_like(rw), regime, n_rows) if rw.numel() else (0.0, 0.0, 0.0)
        print(f'[softmax {regime:8s} rows {n_rows:2d}] fp32 restatement: alpha {ea:.2e}  de {ed:.2e}  row sum {es:.2e}   '
              f'pairwise rows: alpha {ew:.2e}  row sum {esw:.2e}   bounds {ba:.2e} / {bd:.2e}')
        assert ea <= C.SOFTMAX_FLOOR and ed <= C.SOFTMAX_FLOOR
        assert ea <= ba and ed <= bd and ew <= ba and esw <= ba


def test_hub_graph_has_its_hubs_multi_edges_loops_and_isolated_rows():
    ei, et = C.hub_graph()
    n = C.N_NODES
    indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
    assert 1500 <= int(indeg[C.HUB_IN]) < 1520 and int(indeg.argmax()) == C.HUB_IN
    assert 1000 <= int(outdeg[C.HUB_OUT]) < 1020 and int(outdeg.argmax()) == C.HUB_OUT
    assert int(indeg[n - C.N_ISOLATED:].sum()) == 0 and int(outdeg[n - C.N_ISOLATED:].sum()) > 0
    assert int(indeg[:n - C.N_ISOLATED].max()) > 64                                  # a row longer than a wave
    rel = torch.bincount(et, minlength=C.N_REL)
    assert int(rel[-1]) == 0 and int(rel[:-1].min()) > 800                           # the last relation has no edge
    key = (et * n + ei[1]) * n + ei[0]
    assert ei.shape[1] - int(key.unique().numel()) >= 100                            # multi-edges of one relation
    assert int((ei[0] == ei[1]).sum()) >= len(C.SELF_LOOPS)
    assert ei.shape[1] == et.numel() == 1500 + 1000 + 3000 + 100 + len(C.SELF_LOOPS)


@pytest.mark.parametrize('d_in,d_out,nb', C.KERNEL_SHAPES + C.FALLBACK_SHAPES)
def test_fp32_rgat_conv_is_inside_the_gpu_bounds(d_in, d_out, nb):
    ei, et = C.hub_graph()
    c = C.layer_case(d_in, d_out, nb)
    assert all(v.dtype == torch.float32 for v in c.values()) and float(c['bias'].abs().min()) > 0
    assert ei.shape[1] * c['weight'][0].numel() * 8 < 256e6                           # the oracle's weight[edge_type] in fp64
    r64 = C.layer_reference_fp64(d_in, d_out, nb)
    assert torch.equal(r64['y'][C.N_NODES - C.N_ISOLATED:], c['bias'].double().expand(C.N_ISOLATED, -1))
    assert float(r64['dweight'][-1].abs().max()) == 0.0 and float(r64['dweight'][0].abs().max()) > 0
    d = C.layer_fp32_distances(d_in, d_out, nb)
    print(f'[rgat_conv {d_in}->{d_out} blocks {nb}] logit span {r64["span"]:.1f}; fp32 oracle to fp64: '
          + '  '.join(f'{k} {v:.2e}' for k, v in d.items()))
    assert d['y'] < C.TOL
    assert all(d['d' + n] < C.GRAD_TOL for n in C.GRAD_NAMES)


def test_wide_logit_variant_spans_twice_the_range_of_fp32_exp():
    d_in, d_out, nb = C.WIDE_SHAPE
    plain, wide = C.layer_case(d_in, d_out, nb), C.layer_case(d_in, d_out, nb, True)
    assert torch.equal(wide['q'], plain['q'] * 4) and torch.equal(wide['k'], plain['k'] * 4)
    assert all(torch.equal(wide[n], plain[n]) for n in ('x', 'weight', 'bias', 'gy'))
    r64 = C.layer_reference_fp64(d_in, d_out, nb, True)
    d = C.layer_fp32_distances(d_in, d_out, nb, True)
    print(f'[rgat_conv wide logits] span {r64["span"]:.1f} (plain {C.layer_reference_fp64(d_in, d_out, nb)["span"]:.1f}); '
          'fp32 oracle to fp64: ' + '  '.join(f'{k} {v:.2e}' for k, v in d.items()))
    assert r64['span'] > C.WIDE_MIN_SPAN
    assert d['y'] < C.TOL
    assert all(d['d' + n] < C.GRAD_TOL for n in C.GRAD_NAMES)                        # the GPU bound is max(2e-5, 3 x this)


def test_large_graph_reaches_the_second_sweep():
    ei, et = C.large_graph()
    assert C.LARGE_N == 65545 and 3900 <= ei.shape[1] <= 4100 and int(ei.max()) < C.LARGE_N
    for side in (0, 1):                                                               # sources (dx rows) and targets (y rows)
        rows = ei[side]
        assert int((rows >= C.SWEEP).sum()) > 300 and int((rows < 11).sum()) > 300
        assert set(range(C.SWEEP, C.LARGE_N)) <= set(rows.tolist())                   # every row of the second sweep
        assert int(((rows >= C.LARGE_N - 15) & (rows < C.SWEEP)).sum()) > 100         # and the last rows of the first
    assert int(torch.bincount(et, minlength=C.LARGE_REL)[-1]) == 0
    for d_in, d_out, nb in C.LARGE_SHAPES:
        r64 = C.large_reference_fp64(d_in, d_out, nb)
        assert float(r64['y'][C.SWEEP:].abs().min()) > 0 and float(r64['dx'][C.SWEEP:].abs().min()) > 0
        d = C.large_fp32_distances(d_in, d_out, nb)
        print(f'[typed conv n = {C.LARGE_N} {d_in}->{d_out} blocks {nb}] fp32 formula to fp64: '
              + '  '.join(f'{k} {v:.2e}' for k, v in d.items()))
        assert max(d.values()) < C.GRAD_TOL
        r32 = C._large_reference(d_in, d_out, nb, torch.float32)
        assert rel_l2(r32['y'][C.SWEEP:], r64['y'][C.SWEEP:]) < C.GRAD_TOL and rel_l2(r32['dx'][C.SWEEP:], r64['dx'][C.SWEEP:]) < C.GRAD_TOL


def test_fp32_two_layer_oracle_is_inside_the_gpu_bounds():
    state, mask1, mask2, u1, u2 = C.model_case()
    assert bool(mask1[C.HUB_IN]) and bool(mask1[C.HUB_OUT]) and bool(mask2[C.HUB_IN]) and bool(mask2[C.HUB_OUT])
    iso = slice(C.N_NODES - C.N_ISOLATED, C.N_NODES)
    assert 0 < int(mask1[iso].sum()) < C.N_ISOLATED and 0 < int(mask2[iso].sum()) < C.N_ISOLATED
    assert state['conv1.weight'].shape == (2 * C.MODEL_EDGE_TYPES, 4, 16, 32) and float(state['conv2.bias'].abs().min()) > 0
    r64 = C.model_reference_fp64()
    got = {n for n, g in r64['del']['grads'].items() if g is not None}
    assert got == {n for n in C.MODEL_PARAMS if not n.startswith(('conv1', 'node_emb'))}      # conv1 is frozen under Del
    assert {n for n, g in r64['backbone']['grads'].items() if g is not None} == set(C.MODEL_PARAMS[2:])
    d = C.model_fp32_distances()
    print('[two-layer RGATDelete] fp32 oracle to fp64: ' + '  '.join(f'{k} {v:.2e}' for k, v in d.items()))
    for k, v in d.items():
        assert v < (C.TOL if k.endswith(('.z1', '.z2')) else C.GRAD_TOL), (k, v)
