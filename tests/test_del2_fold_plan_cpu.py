"""engine.plan_del2_fold - does the fused Del-2 pass fold W_D2 into conv2's weight? - and its switch, without a GPU or the library."""
import itertools

from gnndelete_amd.engine import Knobs, plan_del2_fold, plan_step, read_del2_fold
from test_step_plan_cpu import MODES, all_facts, headline


def _fold(facts, knobs=Knobs(), covers=True, enabled=True):
    return plan_del2_fold(facts, plan_step(facts, knobs), covers, enabled)


def test_headline_requests():
    for mode in MODES:
        for rows_only in (False, True):
            f = headline(mode, rows_only_asked=rows_only, closed=rows_only and mode != 'rgcn')
            assert _fold(f) == (mode in ('gcn', 'gin')), (mode, rows_only)      # GAT chains too, but its backward needs dp2 itself
            assert not _fold(f, covers=False) and not _fold(f, enabled=False)


def test_each_condition_switches_it_off():
    f = headline('gcn')
    assert _fold(f)
    assert not _fold(f, Knobs(del1_chain=False))                     # not chained: dh is formed from dp2 at the end of the step
    assert not _fold(f, Knobs(no_fused_wgrad2=True))                 # the partials do not come out of the Del-2 kernel
    assert not _fold(f, Knobs(no_fused_l2=True))
    assert not _fold(f, Knobs(no_step_tail=True))
    for lt in ('both_all', 'only1', 'only2_layerwise', 'only2_all'):
        assert not _fold(headline('gcn', loss_type=lt)), lt
    assert not _fold(headline('gcn', family='kld'))
    assert not _fold(headline('gcn', del1_covers=False))
    # a layer-2 loss row outside the Del rows takes the identity: W_D2^T W2 would apply W_D2 to it
    outside = headline('gcn', inside2=False)
    forms = plan_step(outside, Knobs())
    assert forms.out2 and forms.chain1 and forms.fuse_wg2 and not plan_del2_fold(outside, forms, True)


def test_fold_implies_its_conditions_over_the_product_of_facts():
    n = on = 0
    for f in itertools.islice(all_facts(('gcn', 'gin', 'gat')), 0, None, 7):
        r = plan_step(f, Knobs())
        got = plan_del2_fold(f, r, True)
        assert isinstance(got, bool)
        assert got == (r.chain1 and f.mode in ('gcn', 'gin') and r.fuse_wg2 and not r.out2)
        if got:            # what the chained Del-1 pass and the fused Del-2 kernel need
            assert f.loss_type == 'both_layerwise' and f.family == 'mse' and (f.h, f.o) == (128, 64) and r.fuse_l2 and r.tail and r.split2
        n += 1
        on += got
    assert n > 1000 and on > 0


def test_switch_is_read_from_the_environment():
    assert read_del2_fold({}) is True
    assert read_del2_fold({'GD_DEL2_FOLD': '0'}) is False
    assert read_del2_fold({'GD_DEL2_FOLD': '1'}) is True
    assert 'del2_fold' not in Knobs._fields                             # (the recorded form tables spell the Knobs out)
