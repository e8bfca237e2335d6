"""NodeembEngine with conv1's explicit rows formed inside conv2's Linear launch (engine.plan_explicit_chain,
gd_rows_gemm_select_chain_f32) on the 80,001-node biased request of test_layer1_fold_engine_gpu.py (128 -> 128 -> 64, 70,451 Del-1
rows, 9,550 explicit rows, a non-zero conv1 bias), six iterations.

Bars: against GD_EXPLICIT_CHAIN=0 from the same state at bar (e) of test_engine_large_forms_gpu.py for two forms of one step (loss
log rtol 1e-5, weights 2e-5 rel-L2); the fp64 oracle within 1e-4 on every train_loss and on both Del weights; eager, replayed and
run(unroll=4) bit for bit; pre1 is zero on the Del-1 rows and written on every explicit row; no ops.rows_gemm call on the explicit
rows (one with the switch off: the probe has teeth).
"""
import functools

import pytest
import torch

from test_engine_large_forms_gpu import ALPHA, ITERS, LR, _device_request, large_request
from test_layer1_fold_engine_gpu import _biased_state, _oracle64

pytestmark = pytest.mark.gpu


def _engine(chain, graph=False):
    from gnndelete_amd.engine import NodeembEngine
    from helpers import hip_model
    data, _, ni1, ni2 = large_request()
    d = _device_request()
    model = hip_model('gcn', _biased_state('gcn'), data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
    with torch.no_grad():
        z1o, z2o = model.get_original_embeddings(d['x'], d['e_dr'], return_all_emb=True)
    with pytest.MonkeyPatch.context() as mp:               # read in the constructor, once
        mp.setenv('GD_LAYER1_FOLD', '1')
        mp.setenv('GD_EXPLICIT_CHAIN', '1' if chain else '0')
        eng = NodeembEngine(model, d['x'], d['e_sdf'], z1o, z2o, d['pos'], d['neg'], ni1, ni2, loss_type='both_layerwise', alpha=ALPHA, lr=LR,
                            use_graph=graph)
    assert eng._fold1 and eng._chain_expl == chain and eng._idx1c.numel() == eng.n - eng.s1 > 0
    return eng, model


@functools.lru_cache(maxsize=None)
def _run(chain, graph=False, unroll=0):
    eng, model = _engine(chain, graph=graph)
    if unroll:
        eng.run(ITERS, unroll=unroll)
    else:
        for _ in range(ITERS):
            eng.step()
    torch.cuda.synchronize()
    return dict(hist=eng.loss_history(), w=(model.deletion1.deletion_weight.detach().cpu().clone(), model.deletion2.deletion_weight.detach().cpu().clone()),
                replayed=eng._graph is not None, pre1_s1=float(eng.pre1[eng.idx1.long()].abs().max()),
                pre1_rest=float(eng.pre1[eng._idx1c.long()].abs().max(1).values.min()),
                pre1_err=float((eng.pre1[eng._idx1c.long()].double()
                                - (eng._a1[eng._idx1c.long()].double() @ eng._w1.double().t() + eng._b1.double())).abs().max()))


def test_against_the_switch_off_from_the_same_state():
    from helpers import rel_l2
    a, b = _run(True), _run(False)
    d = [rel_l2(x.double(), y.double()) for x, y in zip(a['w'], b['w'])]
    print(f'[explicit chain engine] MEASURED vs GD_EXPLICIT_CHAIN=0: loss {float(((a["hist"][:, 0] - b["hist"][:, 0]) / b["hist"][:, 0]).abs().max()):.1e}, '
          f'W_D1 {d[0]:.1e}, W_D2 {d[1]:.1e}')
    assert a['hist'].shape[0] == b['hist'].shape[0] == ITERS
    assert torch.allclose(a['hist'][:, 0], b['hist'][:, 0], rtol=1e-5, atol=0), (a['hist'][:, 0], b['hist'][:, 0])
    assert d[0] < 2e-5 and d[1] < 2e-5


def test_against_the_fp64_oracle():
    from helpers import rel_l2
    got = _run(True)
    logs, w1, w2 = _oracle64()
    d_loss = max(abs(float(got['hist'][i, 0]) - want) / abs(want) for i, want in enumerate(logs))
    e1, e2 = rel_l2(got['w'][0].double(), w1), rel_l2(got['w'][1].double(), w2)
    print(f'[explicit chain engine] MEASURED to the fp64 oracle after {ITERS} iterations: loss {d_loss:.1e}, W_D1 {e1:.1e}, W_D2 {e2:.1e}')
    assert got['hist'].shape[0] == ITERS
    assert d_loss <= 1e-4 and e1 < 1e-4 and e2 < 1e-4


def test_pre1_is_conv1_on_the_explicit_rows_and_zero_on_the_del1_rows():
    for got in (_run(True), _run(True, graph=True)):
        assert got['pre1_s1'] == 0.0 and got['pre1_rest'] > 0.0
        assert got['pre1_err'] < 1e-4                       # (values of order 1: a 128-term fp32 product against fp64)


def test_replay_and_unrolled_replay_are_the_eager_bits():
    eager, replay, unrolled = _run(True), _run(True, graph=True), _run(True, graph=True, unroll=4)
    assert not eager['replayed'] and replay['replayed'] and unrolled['replayed']
    for other in (replay, unrolled):
        assert torch.equal(other['hist'], eager['hist'])
        assert torch.equal(other['w'][0], eager['w'][0]) and torch.equal(other['w'][1], eager['w'][1])
        assert other['pre1_s1'] == 0.0 and other['pre1_rest'] == eager['pre1_rest']


@pytest.mark.parametrize('chain', [True, False])
def test_no_row_product_on_the_explicit_rows(chain, monkeypatch):
    from gnndelete_amd import ops
    eng, _ = _engine(chain)
    seen, real = [], ops.rows_gemm

    def probe(inp, idx, *a, **k):
        seen.append(idx is eng._idx1c)
        return real(inp, idx, *a, **k)
    monkeypatch.setattr(ops, 'rows_gemm', probe)
    eng.step()
    torch.cuda.synchronize()
    assert any(seen) == (not chain)
