"""The engine with the Del-2 input gradient folded into conv2's weight (engine.plan_del2_fold; GD_DEL2_FOLD=0 switches it off)
against the same engine without, on the request of test_engine_large_forms_gpu.py (80,001 nodes, 128 -> 128 -> 64, s1 = 70,451,
s2 = 72,648: just inside the chained forms) with its seeded Del weights (W_D2 = 0.7 I + 0.05 randn: not symmetric).

  - iteration 0 has no carried gradient and iteration 1's losses are taken before its carried gradient reaches a weight, so the
    losses of iterations 0 and 1 and W_D2 after iteration 0 are the same bits with and without the fold;
  - after ITERS iterations the folded engine's W_D1 / W_D2 are no further from the fp64 oracle than twice the unfolded engine's.
The fp64 oracle is the one test_engine_large_forms_gpu.py computes (shared through its cache).
"""
import pytest
import torch

import test_engine_large_forms_gpu as LF

pytestmark = pytest.mark.gpu

ITERS = LF.ITERS
# (gnn, engine options, captured with two iterations per graph launch)
CASES = {'gcn/eager': ('gcn', 'plain', False), 'gcn/captured': ('gcn', 'plain', True), 'gin/eager': ('gin', 'plain', False),
         'gcn/rows': ('gcn', 'rows', False)}


def _engine(gnn, opts, graph, monkeypatch, fold, ni2=None, model_out=None):
    from gnndelete_amd.engine import NodeembEngine
    from helpers import hip_model
    data, _, ni1, ni2_ = LF.large_request()
    d = LF._device_request()
    model = hip_model(gnn, LF._state(gnn), data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
    with torch.no_grad():
        z1o, z2o = model.get_original_embeddings(d['x'], d['e_dr'], return_all_emb=True)
    with monkeypatch.context() as mp:              # the engine reads the switch in its constructor, once
        if fold:
            mp.delenv('GD_DEL2_FOLD', raising=False)
        else:
            mp.setenv('GD_DEL2_FOLD', '0')
        eng = NodeembEngine(model, d['x'], d['e_sdf'], z1o, z2o, d['pos'], d['neg'], ni1, ni2_ if ni2 is None else ni2, loss_type='both_layerwise',
                            alpha=LF.ALPHA, lr=LF.LR, use_graph=graph, **LF.OPTS[opts])
    return eng, model


def _run(name, monkeypatch, fold):
    gnn, opts, graph = CASES[name]
    eng, model = _engine(gnn, opts, graph, monkeypatch, fold)
    assert eng._fold2 == fold and eng._chain1 and eng._fuse_wg2 and not eng._out2 and eng.s1 >= 65536
    assert (eng._w2fold is not None) == fold
    if fold:
        assert any(t is eng._w2fold for t in eng._mutable_state()), 'the capture warm-up must restore W\''
        assert eng._w2fold.shape == (LF.OUT, LF.HID) and float(eng._w2fold.abs().max()) == 0.0
    eng.step()
    wd2_after_0 = model.deletion2.deletion_weight.detach().clone()
    if graph:
        eng.run(ITERS - 1, unroll=2)               # two two-iteration launches and a single one
        assert eng._graph_k is not None and eng._graph_k[0] == 2
    else:
        for _ in range(ITERS - 1):
            eng.step()
    if fold:                                       # W' of the last iteration: the W_D2 that iteration's rows used (one Adam step back)
        assert bool(torch.isfinite(eng._w2fold).all()) and float(eng._w2fold.abs().max()) > 0
    return dict(hist=eng.loss_history(), wd2_0=wd2_after_0.cpu(),
                w=(model.deletion1.deletion_weight.detach().double().cpu(), model.deletion2.deletion_weight.detach().double().cpu()))


@pytest.mark.parametrize('name', list(CASES))
def test_fold_on_against_fold_off(name, monkeypatch):
    from helpers import rel_l2
    on, off = _run(name, monkeypatch, True), _run(name, monkeypatch, False)
    assert on['hist'].shape[0] == ITERS
    assert torch.equal(on['hist'][:2], off['hist'][:2]), (on['hist'][:2], off['hist'][:2])
    assert torch.equal(on['wd2_0'], off['wd2_0'])
    ref = LF._oracle(CASES[name][0], 'both_layerwise', 'mse_mean')
    for k, wname in enumerate(('W_D1', 'W_D2')):
        e_on, e_off = rel_l2(on['w'][k], ref['w'][k]), rel_l2(off['w'][k], ref['w'][k])
        print(f'[{name}] MEASURED {wname} rel-L2 to the fp64 oracle after {ITERS} iterations: folded {e_on:.3e}, unfolded {e_off:.3e}; '
              f'the two {rel_l2(on["w"][k], off["w"][k]):.3e} apart')
        assert e_on <= 2.0 * e_off, f'{wname}: folded {e_on:.3e}, unfolded {e_off:.3e}'
    for i, want in enumerate(ref['logs']):
        assert abs(float(on['hist'][i, 0]) - want) <= 1e-4 * abs(want), (i, float(on['hist'][i, 0]), want)


def test_fold_is_off_with_a_layer2_loss_row_outside_the_del_rows(monkeypatch):
    data, _, _, ni2 = LF.large_request()
    outside = (~data.sdf_node_2hop_mask).nonzero().flatten()
    assert outside.numel() > 0
    ni2 = ni2.clone()
    ni2[outside[0]] = True
    eng, _ = _engine('gcn', 'plain', False, monkeypatch, True, ni2=ni2)
    assert eng._out2 and eng._chain1 and eng._fuse_wg2 and not eng._fold2 and eng._w2fold is None


def test_fold_is_off_for_gat(monkeypatch):
    eng, _ = _engine('gat', 'plain', False, monkeypatch, True)
    assert eng._chain1 and eng._fuse_wg2 and not eng._fold2 and eng._w2fold is None
