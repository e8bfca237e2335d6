"""engine.plan_layer1_fold - does the chained GCN step fold conv1's weight into W_D1? - and its switch, without a GPU or the library."""
import itertools

from gnndelete_amd.engine import Knobs, StepForms, plan_layer1_fold, plan_step, read_layer1_fold
from test_step_plan_cpu import MODES, all_facts, headline


def _fold(facts, knobs=Knobs(), covers=True, enabled=True):
    return plan_layer1_fold(facts, plan_step(facts, knobs), covers, enabled)


def test_headline_requests():
    for mode in MODES:
        for rows_only in (False, True):
            f = headline(mode, rows_only_asked=rows_only, closed=rows_only and mode != 'rgcn')
            assert _fold(f) == (mode == 'gcn'), (mode, rows_only)     # GIN / GAT chain too: the algebra is wired for GCNConv alone
            assert not _fold(f, covers=False) and not _fold(f, enabled=False)


def test_each_condition_switches_it_off():
    f = headline('gcn')
    assert _fold(f)
    for mode in MODES:
        if mode != 'gcn':
            assert not _fold(headline(mode)), mode
    for lt in ('both_all', 'only1', 'only2_layerwise', 'only2_all'):
        assert not _fold(headline('gcn', loss_type=lt)), lt
    assert not _fold(headline('gcn', cache_layer1=True))             # conv1's output is a fixed buffer then: nothing left to save
    assert not _fold(f, Knobs(del1_chain=False))                     # not chained
    assert not _fold(headline('gcn', del1_covers=False))
    assert not _fold(headline('gcn', family='kld'))
    for h in (32, 64):
        assert not _fold(headline('gcn', h=h)), h
    assert not _fold(f, covers=False)
    assert not _fold(f, enabled=False)
    # the width is checked on its own, not only through chain1
    forms = plan_step(f, Knobs())
    assert forms.chain1 and plan_layer1_fold(f, forms, True) and not plan_layer1_fold(f._replace(h=64), forms, True)
    assert not plan_layer1_fold(f, forms._replace(split1=False), True)
    assert not plan_layer1_fold(f, forms._replace(chain1=False), True)


def test_pure_and_implied_conditions_over_the_product_of_facts():
    n = on = 0
    for f in itertools.islice(all_facts(('gcn', 'gin', 'gat')), 0, None, 7):
        r = plan_step(f, Knobs())
        got = plan_layer1_fold(f, r, True)
        assert isinstance(got, bool) and got == plan_layer1_fold(f, r, True)
        assert isinstance(r, StepForms) and r == plan_step(f, Knobs())           # (the plan was not touched)
        assert got == (r.chain1 and r.split1 and f.mode == 'gcn' and not f.cache_layer1 and f.h == 128)
        if got:
            assert f.loss_type == 'both_layerwise' and f.family == 'mse' and r.fuse_del1 and r.tail and f.del1_covers
        n += 1
        on += got
    assert n > 1000 and on > 0


def test_switch_is_read_from_the_environment():
    assert read_layer1_fold({}) is True
    assert read_layer1_fold({'GD_LAYER1_FOLD': '0'}) is False
    assert read_layer1_fold({'GD_LAYER1_FOLD': '1'}) is True
    assert 'layer1_fold' not in Knobs._fields and 'fold1' not in StepForms._fields      # (the recorded form tables spell both out)
