"""NodeembEngine with conv1's weight folded into W_D1 (engine.plan_layer1_fold) on the 80,001-node request of
test_engine_large_forms_gpu.py (128 -> 128 -> 64, s1 = 70,451 Del-1 rows: the smallest size class the folded kernels cover), with a
NON-ZERO conv1 bias - the synthetic backbones start it at zero, and with b1 = 0 the bias row b1 W_D1 of the folded Del-1 pass and
the b1^T (1^T g) term of dW_D1 would be dead code.

Bars: the fp64 oracle at the trajectory bar of the large-forms test (rel-L2 < 1e-4 on both Del weights, rtol 1e-4 on every train_loss);
folded against GD_LAYER1_FOLD=0 from the same state at that test's bar (e) for two forms of one step (loss log rtol 1e-5, weights
2e-5 rel-L2); eager against replayed and run(unroll=4) against single steps bit for bit, as for every other form.
"""
import functools

import pytest
import torch

from test_engine_large_forms_gpu import ALPHA, F, HID, ITERS, LR, OUT, _device_request, _state, large_request

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _biased_state(gnn='gcn'):
    st = {k: v.clone() for k, v in _state(gnn).items()}
    g = torch.Generator().manual_seed(41)
    assert float(st['conv1.bias'].abs().max()) == 0.0
    st['conv1.bias'] = 0.1 * torch.randn(HID, generator=g)
    return st


@functools.lru_cache(maxsize=None)
def _oracle64():
    from helpers import oracle_runner
    data, neg, ni1, ni2 = large_request()
    step, snap, _ = oracle_runner('gcn', data, _biased_state(), neg, ni1, ni2, torch.float64, torch.device('cuda'), loss_type='both_layerwise',
                                  alpha=ALPHA, lr=LR, hidden=HID, out=OUT)
    logs = [step()['train_loss'] for _ in range(ITERS)]
    w1, w2 = snap()[:2]
    return logs, w1, w2


def _engine(fold, gnn='gcn', graph=False, **opts):
    from gnndelete_amd.engine import NodeembEngine
    from helpers import hip_model
    data, _, ni1, ni2 = large_request()
    d = _device_request()
    model = hip_model(gnn, _biased_state(gnn) if gnn == 'gcn' else _state(gnn), data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
    with torch.no_grad():
        z1o, z2o = model.get_original_embeddings(d['x'], d['e_dr'], return_all_emb=True)
    with pytest.MonkeyPatch.context() as mp:               # read in the constructor, once
        mp.setenv('GD_LAYER1_FOLD', '1' if fold else '0')
        eng = NodeembEngine(model, d['x'], d['e_sdf'], z1o, z2o, d['pos'], d['neg'], ni1, ni2, loss_type='both_layerwise', alpha=ALPHA, lr=LR,
                            use_graph=graph, **opts)
    return eng, model


@functools.lru_cache(maxsize=None)
def _run(fold, graph=False, unroll=0):
    eng, model = _engine(fold, graph=graph)
    assert eng._chain1 and eng._fuse_del1 and eng._split1 and eng._fold1 == fold and eng.x.shape[1] == F
    if fold:
        assert eng._idx1c.numel() == eng.n - eng.s1 and float(eng.pre1.abs().max()) == 0.0
    else:
        assert not hasattr(eng, '_a1') and not hasattr(eng, '_wf')
    if unroll:
        eng.run(ITERS, unroll=unroll)
    else:
        for _ in range(ITERS):
            eng.step()
    torch.cuda.synchronize()
    out = dict(hist=eng.loss_history(), w=(model.deletion1.deletion_weight.detach().cpu().clone(), model.deletion2.deletion_weight.detach().cpu().clone()),
               g1=eng.g1.cpu().clone(), replayed=eng._graph is not None)
    if fold:
        # the carried fold is the fold of the weight the run ended with, and pre1 was never written on the Del-1 rows
        out['wf_err'] = float((eng._wf.double() - eng._w1.double().t() @ eng.wd1.detach().double()).norm() / eng._wf.double().norm())
        out['bf_err'] = float((eng._bf.double() - eng._b1.double() @ eng.wd1.detach().double()).norm() / eng._bf.double().norm())
        out['pre1_s1'] = float(eng.pre1[eng.idx1.long()].abs().max())
        out['pre1_rest'] = float(eng.pre1[eng._idx1c.long()].abs().max(1).values.min())      # (> 0: every other row was)
    return out


def test_folded_engine_against_the_fp64_oracle():
    from helpers import rel_l2
    got = _run(True)
    logs, w1, w2 = _oracle64()
    d_loss = max(abs(float(got['hist'][i, 0]) - want) / abs(want) for i, want in enumerate(logs))
    e1, e2 = rel_l2(got['w'][0].double(), w1), rel_l2(got['w'][1].double(), w2)
    print(f'[layer-1 fold engine] MEASURED to the fp64 oracle after {ITERS} iterations: loss {d_loss:.1e}, W_D1 {e1:.1e}, W_D2 {e2:.1e}; '
          f'carried Wf {got["wf_err"]:.1e}, bf {got["bf_err"]:.1e}')
    assert got['hist'].shape[0] == ITERS
    for i, want in enumerate(logs):
        assert abs(float(got['hist'][i, 0]) - want) <= 1e-4 * abs(want), (i, float(got['hist'][i, 0]), want)
    assert e1 < 1e-4 and e2 < 1e-4
    assert got['wf_err'] <= 1e-5 and got['bf_err'] <= 1e-5
    assert got['pre1_s1'] == 0.0 and got['pre1_rest'] > 0.0


def test_the_bias_matters_at_this_bar():
    """Teeth: the fp64 oracle of the same request with b1 = 0 is further from the biased one than ten times the bars."""
    from helpers import oracle_runner, rel_l2
    data, neg, ni1, ni2 = large_request()
    step, snap, _ = oracle_runner('gcn', data, _state('gcn'), neg, ni1, ni2, torch.float64, torch.device('cuda'), loss_type='both_layerwise',
                                  alpha=ALPHA, lr=LR, hidden=HID, out=OUT)
    logs0 = [step()['train_loss'] for _ in range(ITERS)]
    logs, w1, _ = _oracle64()
    d_loss, d_w = abs(logs0[-1] - logs[-1]) / abs(logs[-1]), rel_l2(snap()[0], w1)
    print(f'[layer-1 fold engine] the oracle without the bias: last loss {d_loss:.1e} away, W_D1 {d_w:.1e}')
    assert d_loss > 1e-3 and d_w > 1e-3


def test_folded_against_unfolded_from_the_same_state():
    from helpers import rel_l2
    a, b = _run(True), _run(False)
    d = [rel_l2(x.double(), y.double()) for x, y in zip(a['w'], b['w'])]
    print(f'[layer-1 fold engine] MEASURED folded vs GD_LAYER1_FOLD=0: loss {float(((a["hist"][:, 0] - b["hist"][:, 0]) / b["hist"][:, 0]).abs().max()):.1e}, '
          f'W_D1 {d[0]:.1e}, W_D2 {d[1]:.1e}, last dW_D1 {rel_l2(a["g1"].double(), b["g1"].double()):.1e}')
    assert torch.allclose(a['hist'][:, 0], b['hist'][:, 0], rtol=1e-5, atol=0), (a['hist'][:, 0], b['hist'][:, 0])
    assert d[0] < 2e-5 and d[1] < 2e-5
    assert rel_l2(a['g1'].double(), b['g1'].double()) < 1e-4           # self.g1 holds the true gradient W1 G + b1^T s


def test_replay_and_unrolled_replay_are_the_eager_bits():
    eager, replay, unrolled = _run(True), _run(True, graph=True), _run(True, graph=True, unroll=4)
    assert not eager['replayed'] and replay['replayed'] and unrolled['replayed']
    for other in (replay, unrolled):
        assert torch.equal(other['hist'], eager['hist'])
        assert torch.equal(other['w'][0], eager['w'][0]) and torch.equal(other['w'][1], eager['w'][1])
        assert other['wf_err'] == eager['wf_err'] and other['pre1_s1'] == 0.0


@pytest.mark.parametrize('gnn,opts', [('gcn', dict(cache_layer1=True)), ('gat', {})])
def test_fold_falls_away(gnn, opts):
    eng, _ = _engine(True, gnn=gnn, **opts)
    assert eng._chain1 and not eng._fold1 and not hasattr(eng, '_a1') and not hasattr(eng, '_idx1c')
    eng.step()
    torch.cuda.synchronize()
    assert float(eng.pre1[eng.idx1.long()].abs().max()) > 0.0           # conv1's output on the Del-1 rows: the unfolded step's operand
    assert eng.loss_history().shape[0] == 1
