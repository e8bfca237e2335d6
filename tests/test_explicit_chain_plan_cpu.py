"""engine.plan_explicit_chain - does the folded GCN step form conv1's explicit rows inside conv2's Linear launch? - its switch, and
the launches the two pieces of the step (_conv1_forward, _linear_relu_z1) make either way; without a GPU or the library."""
import itertools
from types import SimpleNamespace

import torch

from gnndelete_amd import engine, ops
from gnndelete_amd.engine import Knobs, StepForms, plan_explicit_chain, plan_layer1_fold, plan_step, read_explicit_chain
from test_step_plan_cpu import MODES, all_facts, headline


def _chain(facts, knobs=Knobs(), covers=True, enabled=True, fold_covers=True, n_explicit=56947):
    forms = plan_step(facts, knobs)
    fold1 = plan_layer1_fold(facts, forms, fold_covers, True)
    return plan_explicit_chain(facts, forms, covers, enabled, fold1=fold1, n_explicit=n_explicit)


def test_headline_requests():
    for mode in MODES:
        for rows_only in (False, True):
            f = headline(mode, rows_only_asked=rows_only, closed=rows_only and mode != 'rgcn')
            assert _chain(f) == (mode == 'gcn' and not rows_only), (mode, rows_only)
            assert not _chain(f, covers=False) and not _chain(f, enabled=False) and not _chain(f, n_explicit=0)


def test_each_condition_switches_it_off():
    f = headline('gcn')
    assert _chain(f)
    assert not _chain(f, covers=False)                                # the library's coverage query
    assert not _chain(f, enabled=False)                               # GD_EXPLICIT_CHAIN=0
    assert not _chain(f, n_explicit=0)                                # every row is a Del-1 row: nothing explicit to form
    assert not _chain(f, fold_covers=False)                           # not folded: conv1's output is formed on every row
    assert not _chain(headline('gcn', cache_layer1=True))
    assert not _chain(headline('gcn', rows_only_asked=True, closed=True))
    assert not _chain(f, Knobs(del1_chain=False))
    for lt in ('both_all', 'only1', 'only2_layerwise', 'only2_all'):
        assert not _chain(headline('gcn', loss_type=lt)), lt
    # the widths and the mode are checked on their own, not only through the fold
    forms = plan_step(f, Knobs())
    assert plan_explicit_chain(f, forms, True, True, fold1=True, n_explicit=1)
    assert not plan_explicit_chain(f._replace(o=32), forms, True, True, fold1=True, n_explicit=1)
    assert not plan_explicit_chain(f._replace(h=64), forms, True, True, fold1=True, n_explicit=1)
    assert not plan_explicit_chain(f._replace(mode='gin'), forms, True, True, fold1=True, n_explicit=1)
    assert not plan_explicit_chain(f._replace(cache_layer1=True), forms, True, True, fold1=True, n_explicit=1)
    assert not plan_explicit_chain(f, forms._replace(rows_only=True), True, True, fold1=True, n_explicit=1)
    assert not plan_explicit_chain(f, forms, True, True, fold1=False, n_explicit=1)


def test_pure_over_the_product_of_facts():
    n = on = 0
    for f in itertools.islice(all_facts(('gcn', 'gin', 'gat')), 0, None, 7):
        r = plan_step(f, Knobs())
        fold1 = plan_layer1_fold(f, r, True)
        got = plan_explicit_chain(f, r, True, True, fold1=fold1, n_explicit=3)
        assert isinstance(got, bool) and got == plan_explicit_chain(f, r, True, True, fold1=fold1, n_explicit=3)
        assert isinstance(r, StepForms) and r == plan_step(f, Knobs())
        assert got == (fold1 and not r.rows_only and f.o == 64)
        if got:
            assert f.mode == 'gcn' and f.h == 128 and r.chain1 and r.split1 and not f.cache_layer1
        n += 1
        on += got
    assert n > 1000 and on > 0


def test_switch_is_read_from_the_environment():
    assert read_explicit_chain({}) is True
    assert read_explicit_chain({'GD_EXPLICIT_CHAIN': '0'}) is False
    assert read_explicit_chain({'GD_EXPLICIT_CHAIN': '1'}) is True
    assert 'explicit_chain' not in Knobs._fields and 'chain_expl' not in StepForms._fields


def _step_pieces(chain_expl, n_explicit, monkeypatch):
    """The launches _conv1_forward and _linear_relu_z1 make on a folded GCN engine whose planner said chain_expl (a stand-in
    object with the attributes the two methods read; every op is recorded, none runs)."""
    calls = []
    w2 = torch.zeros(64, 128)
    eng = SimpleNamespace(
        _mode='gcn', _fold1=True, _chain_expl=chain_expl, _rows_only=False, _split1=True, _plan2=None,
        model=SimpleNamespace(conv1=SimpleNamespace()), graph=SimpleNamespace(val='val'), x='x', _a1='a1', _w1='w1', _b1='b1', pre1='pre1',
        z1='z1', _sel1='sel1', idx1='idx1', _idx1c=torch.zeros(n_explicit, dtype=torch.int32),
        _spmm=lambda *a, **k: calls.append('spmm'), _mfma_weight=lambda w: True)
    monkeypatch.setattr(ops, 'rows_gemm', lambda inp, idx, *a, **k: calls.append(('rows_gemm', inp, idx is eng._idx1c, k.get('out'))))
    monkeypatch.setattr(ops, 'rows_gemm_select', lambda inp, alt, sel, *a, **k: calls.append(('rows_gemm_select', inp, alt, sel)))
    monkeypatch.setattr(ops, 'rows_gemm_select_chain', lambda *a, **k: calls.append(('rows_gemm_select_chain',) + a[:7]))
    engine.NodeembEngine._conv1_forward(eng)
    engine.NodeembEngine._linear_relu_z1(eng, w2)
    return calls, eng


def test_switch_off_and_no_explicit_rows_give_the_parents_step(monkeypatch):
    # the parent's step: aggregation, a W1^T + b1 on the explicit rows into pre1, the selector product over (pre1 | z1)
    parent = ['spmm', ('rows_gemm', 'a1', True, 'pre1'), ('rows_gemm_select', 'pre1', 'z1', 'sel1')]
    off, _ = _step_pieces(plan_explicit_chain(headline('gcn'), plan_step(headline('gcn'), Knobs()), True,
                                              read_explicit_chain({'GD_EXPLICIT_CHAIN': '0'}), fold1=True, n_explicit=5), 5, monkeypatch)
    assert off == parent
    # no explicit rows: the planner says no, and the parent's step then has no explicit-rows launch either
    f = headline('gcn')
    none, _ = _step_pieces(plan_explicit_chain(f, plan_step(f, Knobs()), True, True, fold1=True, n_explicit=0), 0, monkeypatch)
    assert none == ['spmm', ('rows_gemm_select', 'pre1', 'z1', 'sel1')]
    # on: one launch for both, no explicit-rows product of its own
    on, eng = _step_pieces(plan_explicit_chain(f, plan_step(f, Knobs()), True, True, fold1=True, n_explicit=5), 5, monkeypatch)
    assert on[0] == 'spmm' and len(on) == 2 and on[1][0] == 'rows_gemm_select_chain'
    assert on[1][1] == 'a1' and on[1][2] is eng._idx1c and on[1][3:] == ('w1', 'b1', 'pre1', 'z1', 'idx1')
