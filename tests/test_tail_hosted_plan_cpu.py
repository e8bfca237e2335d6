"""engine.plan_tail_hosted - does the step tail ride on the two layer-2 aggregation launches? - its switch, the shape test behind its
`wide` argument and the launches the engine reports either way; without a GPU or the library."""
import itertools
from types import SimpleNamespace

from gnndelete_amd import engine, ops
from gnndelete_amd.engine import (Knobs, StepForms, plan_del2_fold, plan_layer1_fold, plan_step, plan_tail_hosted, read_tail_hosted)
from test_step_plan_cpu import MODES, all_facts, headline


def _hosted(facts, knobs=Knobs(), enabled=True, fold1_covers=True, fold2_covers=True, **kw):
    forms = plan_step(facts, knobs)
    fold1 = plan_layer1_fold(facts, forms, fold1_covers, True)
    fold2 = plan_del2_fold(facts, forms, fold2_covers, True)
    args = dict(fold1=fold1, fold2=fold2, wide=True, padded=False)
    args.update(kw)
    return plan_tail_hosted(facts, forms, enabled, **args)


def test_headline_requests():
    for mode in MODES:
        for rows_only in (False, True):
            f = headline(mode, rows_only_asked=rows_only, closed=rows_only and mode != 'rgcn')
            assert _hosted(f) == (mode == 'gcn' and not rows_only), (mode, rows_only)
            assert not _hosted(f, enabled=False)


def test_each_excluded_condition_switches_it_off():
    f = headline('gcn')
    assert _hosted(f)
    assert not _hosted(f, enabled=False)                               # GD_TAIL_HOSTED=0
    assert not _hosted(f, fold1_covers=False)                          # layer 1 not folded: the tail's job 1 is another kernel
    assert not _hosted(f, fold2_covers=False)                          # layer 2 not folded
    assert not _hosted(f, wide=False)                                  # an aggregation on another form
    assert not _hosted(f, padded=True)                                 # padded class dimension: the copy-back follows the tail
    assert not _hosted(headline('gcn', rows_only_asked=True, closed=True))
    assert not _hosted(headline('gcn', cache_layer1=True))
    assert not _hosted(f, Knobs(no_step_tail=True)) and not _hosted(f, Knobs(del1_chain=False)) and not _hosted(f, Knobs(no_fused_wgrad2=True))
    for lt in ('both_all', 'only1', 'only2_layerwise', 'only2_all'):
        assert not _hosted(headline('gcn', loss_type=lt)), lt
    for family in ('kld', 'cosine'):
        assert not _hosted(headline('gcn', family=family)), family
    # every condition is checked on its own, not only through the folds
    forms = plan_step(f, Knobs())
    on = dict(fold1=True, fold2=True, wide=True, padded=False)
    assert plan_tail_hosted(f, forms, True, **on)
    for k, v in (('fold1', False), ('fold2', False), ('wide', False), ('padded', True)):
        assert not plan_tail_hosted(f, forms, True, **dict(on, **{k: v})), k
    for mode in ('gin', 'gat', 'sage', 'rgcn'):
        assert not plan_tail_hosted(f._replace(mode=mode), forms, True, **on), mode
    assert not plan_tail_hosted(f._replace(loss_type='both_all'), forms, True, **on)
    for field in ('tail', 'chain1', 'fuse_wg2'):
        assert not plan_tail_hosted(f, forms._replace(**{field: False}), True, **on), field
    assert not plan_tail_hosted(f, forms._replace(rows_only=True), True, **on)


def test_pure_over_the_product_of_facts():
    n = on = 0
    for f in itertools.islice(all_facts(('gcn', 'gin', 'gat')), 0, None, 7):
        r = plan_step(f, Knobs())
        fold1, fold2 = plan_layer1_fold(f, r, True), plan_del2_fold(f, r, True)
        got = plan_tail_hosted(f, r, True, fold1=fold1, fold2=fold2, wide=True, padded=False)
        assert isinstance(got, bool) and got == plan_tail_hosted(f, r, True, fold1=fold1, fold2=fold2, wide=True, padded=False)
        assert isinstance(r, StepForms) and r == plan_step(f, Knobs())
        assert got == (fold1 and fold2 and not r.rows_only)
        if got:
            assert f.mode == 'gcn' and f.h == 128 and f.loss_type == 'both_layerwise' and r.tail and r.chain1 and r.fuse_wg2
        n += 1
        on += got
    assert n > 1000 and on > 0


def test_switch_is_read_from_the_environment():
    assert read_tail_hosted({}) is True
    assert read_tail_hosted({'GD_TAIL_HOSTED': '0'}) is False
    assert read_tail_hosted({'GD_TAIL_HOSTED': '1'}) is True
    assert 'tail_hosted' not in Knobs._fields and 'tail_hosted' not in StepForms._fields


def test_wide_form_of_the_shapes():
    big = 235868
    assert ops.spmm_wide_form(64, big, 64, 64, env={})
    assert ops.spmm_wide_form(64, big, 80, 64, env={})
    assert not ops.spmm_wide_form(128, big, 128, 128, env={}) and not ops.spmm_wide_form(32, big, 32, 32, env={})
    assert not ops.spmm_wide_form(64, 1 << 24, 64, 64, env={})                       # row ids need 24 bits
    assert not ops.spmm_wide_form(64, big, 1 << 22, 64, env={})                      # the pitch in bytes, too
    assert not ops.spmm_wide_form(64, (1 << 24) - 1, 80, 64, env={})                 # x above 4 GiB
    for name, value in (('GD_SPMM_TWO_LAUNCH', '1'), ('GD_SPMM_MULTIROW', '0'), ('GD_SPMM_D64_FORM', 'pairs')):
        assert not ops.spmm_wide_form(64, big, 64, 64, env={name: value}), name


def test_the_engine_reports_its_launches_from_the_forms():
    def stages(**kw):
        eng = SimpleNamespace(**dict(dict(_fold1=True, _fold2=True, _chain1=True, _tail=True, _rows_only=False, _chain_expl=True, _tail_hosted=True), **kw))
        return engine.NodeembEngine.step_stages(eng)
    six = ['spmm1', 'del1_loss_wgrad1', 't2', 'spmm2', 'del2_loss_bwd', 'spmm2_t']
    assert stages() == six and stages(_tail_hosted=False) == six + ['tail']
    assert stages(_chain_expl=False, _tail_hosted=False) == ['spmm1', 'pre1_rest'] + six[1:] + ['tail']
    for off in ('_fold1', '_fold2', '_chain1', '_tail'):
        assert stages(**{off: False}) is None
    assert stages(_rows_only=True) is None


def test_no_job_arguments_where_the_tail_has_its_own_launch():
    assert engine.NodeembEngine._tail_host(SimpleNamespace(_tail_hosted=False), 1) is None


def test_the_partitioned_engine_never_hosts():
    """PartitionedNodeembEngine builds its own step: it neither asks the plan nor passes jobs to its aggregations."""
    import inspect
    from gnndelete_amd import dist_engine
    src = inspect.getsource(dist_engine)
    assert 'plan_tail_hosted' not in src and 'host=' not in src and '_tail_host' not in src
