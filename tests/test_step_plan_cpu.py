"""engine.plan_step - the pure function that decides a step's kernel forms - without a GPU or the library: the invariants the
step relies on over the whole product of facts and knobs, the headline requests written out by hand, and the table recorded on
the GPU (tests/golden/engine_forms.json).  Line numbers in the invariants: engine.py of commit d238d52, whose ladder of flags
plan_step replaced."""
import itertools
import json
import os

import pytest

from gnndelete_amd.engine import Knobs, StepFacts, StepForms, padded_class_width, plan_step, read_knobs

MODES = ('gcn', 'gin', 'gat', 'sage', 'rgcn')
LOSS_TYPES = ('both_all', 'both_layerwise', 'only2_layerwise', 'only2_all', 'only1')


def _layer_states(s, family):
    """(folded, n_rows, inside) a layer can be in: a layer that is not folded has no loss rows to speak of and is refused by
    the constructor for KLD / cosine; `inside` is _rows_inside - false without Del rows, true without loss rows."""
    states = [(True, 0, s > 0), (True, 5, False)] + ([(True, 5, True)] if s > 0 else [])
    return states + ([(False, 0, False)] if family == 'mse' else [])


def all_facts(modes=MODES):
    for mode, lt, family in itertools.product(modes, LOSS_TYPES, ('mse', 'kld', 'cosine')):
        if mode == 'rgcn' and family != 'mse':
            continue                                    # (the constructor refuses it)
        for h, o, s1, s2 in itertools.product((32, 48, 64, 128), (16, 32, 64), (0, 1, 70000), (0, 1, 70000)):
            w2_mfma = mode != 'rgcn' and h % 32 == 0 and o % 32 == 0          # (_mfma_weight of an [o, h] weight at these widths)
            pair = h in (64, 128) and o in (64, 128)
            covers = (False, True) if (h == 128 and s1 >= 65536) else (False,)   # (False there too: GD_DEL1_FUSED=0)
            asked_closed = [(False, False), (True, False)] + ([(True, True)] if mode != 'rgcn' and s2 > 0 else [])
            for l1, l2, cache, (asked, closed), gin_ok, cov in itertools.product(
                    _layer_states(s1, family), _layer_states(s2, family), (False, True), asked_closed,
                    (False, True) if mode == 'gin' else (False,), covers):
                yield StepFacts(mode, lt, family, h, o, s1, s2, *l1, *l2, cache, asked, closed, w2_mfma, gin_ok, cov, pair)


# the knobs plan_step reads (the other four select kernels inside a form: the R-GCN order / kernels, GraphSAGE's root term)
PLAN_KNOBS = ('no_split_loss', 'no_split', 'no_fused_l2', 'cache_split', 'no_fused_loss1', 'no_step_tail', 'tail_fused_only',
              'no_fused_wgrad2', 'del1_chain', 'no_gat_rank1_epilogue', 'no_loss_pair', 'no_gat_dots')


def invariants_hold(f, r):
    (split1, split2, out1, out2, fuse_loss1, fuse_l2, tail, fuse_wg2, fuse_del1, chain1, out_pair, rows_only, rgcn_rows_only,
     gat_dots) = r
    return (
        # chain1 => fuse_del1 (:581, :586) => tail and fuse_loss1 and split1 (:572)
        (not chain1 or fuse_del1) and (not fuse_del1 or (tail and fuse_loss1 and split1))
        # fuse_wg2 => tail and fuse_l2 (:564);  fuse_l2 => split2 (:484)
        and (not fuse_wg2 or (tail and fuse_l2)) and (not fuse_l2 or split2)
        # out_pair => out1 and out2 and fuse_loss1 and fuse_l2 (:603)
        and (not out_pair or (out1 and out2 and fuse_loss1 and fuse_l2))
        # rows_only => split2 and not out1 and not out2 (:650-651)
        and (not rows_only or (split2 and not out1 and not out2))
        # a non-MSE family: none of the forms that fuse the MSE loss (`self._mse` in :476, :484, :537 and what follows from them)
        and (f.family == 'mse' or not (fuse_loss1 or fuse_l2 or fuse_wg2 or fuse_del1 or chain1 or out_pair))
        # fuse_del1 => del1_covers (:573)
        and (not fuse_del1 or f.del1_covers)
        # what the buffers and launches of the constructor / _iteration assume on top of the list above:
        and (not out1 or (fuse_loss1 and not split1))      # (:541-543: the outside launch exists next to the fused loss only)
        and (not out2 or split2)                           # (:478-480)
        and (not split1 or f.inside1)                      # (:497-498: the out-of-place Del-1 never forms z1 rows outside S1)
        and rgcn_rows_only == (f.rows_only_asked and f.mode == 'rgcn') and not (rows_only and rgcn_rows_only)
        and set(map(type, r)) == {bool})


@pytest.mark.parametrize('mode', MODES)
def test_invariants_over_the_product_of_facts_and_knobs(mode):
    """Every fact combination that can occur, under the default knobs and with each knob plan_step reads flipped on its own:
    6.2 million calls over the five backbones, a few seconds for each."""
    settings = [Knobs()] + [Knobs()._replace(**{name: not Knobs._field_defaults[name]}) for name in PLAN_KNOBS]
    n = 0
    for f in all_facts((mode,)):
        for k in settings:
            assert invariants_hold(f, plan_step(f, k)), (f, k, plan_step(f, k))
        n += 1
    assert n > 30000


def test_the_other_knobs_do_not_reach_plan_step():
    others = [name for name in Knobs._fields if name not in PLAN_KNOBS]
    assert sorted(others) == ['pad_out', 'rgcn_node_major', 'rgcn_relu_pass', 'rgcn_reorder', 'sage_root_in_spmm']
    for f in itertools.islice(all_facts(), 0, None, 97):
        for name in others:
            flipped = Knobs()._replace(**{name: 32 if name == 'pad_out' else not Knobs._field_defaults[name]})
            assert plan_step(f, flipped) == plan_step(f, Knobs())


def headline(mode, **kw):
    base = dict(mode=mode, loss_type='both_layerwise', family='mse', h=128, o=64, s1=180000, s2=230000, folded1=True, n_rows1=170000,
                inside1=True, folded2=True, n_rows2=220000, inside2=True, cache_layer1=False, rows_only_asked=False, closed=False,
                w2_mfma=mode != 'rgcn', gin_ok=mode == 'gin', del1_covers=True, pair_covers=True)
    return StepFacts(**dict(base, **kw))


@pytest.mark.parametrize('rows_only', [False, True])
@pytest.mark.parametrize('mode', MODES)
def test_headline_request_runs_the_one_pass_forms(mode, rows_only):
    """test_full_size_gpu.py:80-81 and, with affected_rows_only on closed row sets, :97."""
    closed = rows_only and mode != 'rgcn'                # (R-GCN: the option restricts conv2's input gradient instead)
    r = plan_step(headline(mode, rows_only_asked=rows_only, closed=closed), Knobs())
    assert r.fuse_del1 and r.fuse_wg2 and r.tail and r.split1 and r.split2 and r.fuse_loss1 and r.fuse_l2
    assert r.chain1 == (mode in ('gcn', 'gin', 'gat'))
    assert r.rows_only == closed and r.rgcn_rows_only == (rows_only and not closed) and not (r.out1 or r.out2 or r.out_pair)
    assert not plan_step(headline(mode, del1_covers=False), Knobs()).fuse_del1


@pytest.mark.parametrize('family', ['kld', 'cosine'])
def test_row_loss_families_keep_the_tail_and_drop_the_mse_forms(family):
    """test_row_losses_engine_gpu.py:227-232 (the wide and the narrow GAT fixture, 32 -> 128 -> 64 and 10 -> 32 -> 16)."""
    small = dict(s1=300, s2=600, n_rows1=200, n_rows2=400, del1_covers=False)
    r = plan_step(headline('gat', family=family, **small), Knobs())
    assert not (r.fuse_loss1 or r.fuse_l2 or r.fuse_del1 or r.fuse_wg2 or r.chain1 or r.out_pair)
    assert r.tail and r.split1 and r.split2
    mse = plan_step(headline('gat', **small), Knobs())
    assert mse.fuse_loss1 and mse.fuse_l2 and mse.tail
    narrow = plan_step(headline('gat', family=family, h=32, o=16, w2_mfma=False, pair_covers=False, **small), Knobs())
    assert not narrow.tail and not narrow.fuse_loss1


@pytest.mark.parametrize('mode,loss_type', [('gcn', 'both_all'), ('gat', 'both_layerwise')])
def test_knobs_switch_off_what_the_trajectory_tests_expect(mode, loss_type):
    small = dict(loss_type=loss_type, s1=300, s2=600, n_rows1=200, n_rows2=400, del1_covers=False)
    # test_engine_gpu.py:85 - the wide fixtures (32 -> 128 -> 64)
    for knob in (None, 'no_fused_wgrad2', 'no_step_tail'):
        r = plan_step(headline(mode, **small), Knobs()._replace(**({knob: True} if knob else {})))
        assert r.tail == (knob != 'no_step_tail') and r.fuse_wg2 == (knob is None)
    # test_engine_gpu.py:304 - the narrow fixtures (10 -> 32 -> 16)
    narrow = headline(mode, h=32, o=16, w2_mfma=False, pair_covers=False, **small)
    assert plan_step(narrow, Knobs()).split2 and plan_step(narrow, Knobs()).fuse_loss1
    for knob, form in (('no_split', 'split2'), ('no_fused_loss1', 'fuse_loss1'), ('no_fused_l2', 'fuse_l2')):
        assert not getattr(plan_step(narrow, Knobs()._replace(**{knob: True})), form)


def test_recorded_table():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'engine_forms.json')) as f:
        rows = json.load(f)
    assert len(rows) > 100
    for row in rows:
        assert plan_step(StepFacts(**row['facts']), Knobs(**row['knobs'])) == StepForms(**row['forms']), row['case']


def test_knobs_are_read_from_the_environment_once(monkeypatch):
    for name in Knobs._fields:
        monkeypatch.delenv('GD_' + name.upper(), raising=False)
    assert read_knobs() == Knobs()
    monkeypatch.setenv('GD_NO_SPLIT', '1')
    monkeypatch.setenv('GD_DEL1_CHAIN', '0')
    monkeypatch.setenv('GD_PAD_OUT', '32')
    assert read_knobs() == Knobs(no_split=True, del1_chain=False, pad_out=32)
    monkeypatch.setenv('GD_PAD_OUT', 'sixty-four')
    with pytest.warns(UserWarning, match='GD_PAD_OUT'):
        assert read_knobs().pad_out == 0
    with pytest.warns(UserWarning, match='GD_PAD_OUT'):
        assert padded_class_width(128, 4) == 4
