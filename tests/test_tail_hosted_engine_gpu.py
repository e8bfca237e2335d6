"""NodeembEngine with the step tail riding on the two layer-2 aggregation launches (engine.plan_tail_hosted,
gd_spmm_csr_onepass_wide_hosted_f32) on the 80,001-node biased request of test_explicit_chain_engine_gpu.py (128 -> 128 -> 64, a
non-zero conv1 bias), six iterations.

Every comparison is on bits: hosted against GD_TAIL_HOSTED=0 from the same state (Del weights, Adam moments, loss history, the
iteration counter and the ring position); eager, replayed and run(unroll=4).  The engine reports six launches (seven with the switch
off) from its forms, both aggregations carry jobs, and `arrive` is back at 0."""
import functools

import pytest
import torch

from test_engine_large_forms_gpu import ALPHA, ITERS, LR, _device_request, large_request
from test_layer1_fold_engine_gpu import _biased_state

pytestmark = pytest.mark.gpu
SIX = ['spmm1', 'del1_loss_wgrad1', 't2', 'spmm2', 'del2_loss_bwd', 'spmm2_t']


def _engine(hosted, graph=False):
    from gnndelete_amd.engine import NodeembEngine
    from helpers import hip_model
    data, _, ni1, ni2 = large_request()
    d = _device_request()
    model = hip_model('gcn', _biased_state('gcn'), data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
    with torch.no_grad():
        z1o, z2o = model.get_original_embeddings(d['x'], d['e_dr'], return_all_emb=True)
    with pytest.MonkeyPatch.context() as mp:               # read in the constructor, once
        mp.setenv('GD_LAYER1_FOLD', '1')
        mp.setenv('GD_EXPLICIT_CHAIN', '1')
        mp.setenv('GD_TAIL_HOSTED', '1' if hosted else '0')
        eng = NodeembEngine(model, d['x'], d['e_sdf'], z1o, z2o, d['pos'], d['neg'], ni1, ni2, loss_type='both_layerwise', alpha=ALPHA, lr=LR,
                            use_graph=graph)
    assert eng._fold1 and eng._fold2 and eng._chain_expl and eng._tail and eng._tail_hosted == hosted
    return eng, model


@functools.lru_cache(maxsize=None)
def _run(hosted, graph=False, unroll=0):
    eng, model = _engine(hosted, graph=graph)
    if unroll:
        eng.run(ITERS, unroll=unroll)
    else:
        for _ in range(ITERS):
            eng.step()
    torch.cuda.synchronize()
    c = lambda t: t.detach().cpu().clone()
    return dict(hist=eng.loss_history(), raw=c(eng.hist), w1=c(model.deletion1.deletion_weight), w2=c(model.deletion2.deletion_weight),
                m1=c(eng.adam1.m), v1=c(eng.adam1.v), m2=c(eng.adam2.m), v2=c(eng.adam2.v), g1=c(eng.g1), g2=c(eng.g2), wf=c(eng._wf), bf=c(eng._bf),
                iter=int(eng.iter_ctr), pos=int(eng.hist_pos), arrive=c(eng._arrive), applied=(eng.adam1.applied, eng.adam2.applied),
                replayed=eng._graph is not None, stages=eng.step_stages(), cap=int(eng.hist.shape[0]))


BITS = ('hist', 'raw', 'w1', 'w2', 'm1', 'v1', 'm2', 'v2', 'g1', 'g2', 'wf', 'bf', 'arrive')


def test_hosted_is_the_seven_launch_step_bit_for_bit():
    a, b = _run(True), _run(False)
    assert a['hist'].shape[0] == b['hist'].shape[0] == ITERS and bool(torch.isfinite(a['hist'][:, 0]).all())
    for k in BITS:
        assert torch.equal(a[k], b[k]), k
    assert a['iter'] == b['iter'] == ITERS and a['pos'] == b['pos'] == ITERS % a['cap'] and a['applied'] == b['applied'] == (ITERS, ITERS)
    assert int(a['arrive'].abs().sum()) == 0
    assert float(a['m1'].abs().max()) > 0 and float(a['m2'].abs().max()) > 0                # (both optimizers stepped)


def test_replay_and_unrolled_replay_are_the_eager_bits():
    eager, replay, unrolled = _run(True), _run(True, graph=True), _run(True, graph=True, unroll=4)
    assert not eager['replayed'] and replay['replayed'] and unrolled['replayed']
    for other in (replay, unrolled):
        for k in BITS:
            assert torch.equal(other[k], eager[k]), k
        assert other['iter'] == eager['iter'] and other['pos'] == eager['pos']


def test_the_engine_reports_six_launches():
    assert _run(True)['stages'] == SIX and _run(False)['stages'] == SIX + ['tail']


@pytest.mark.parametrize('hosted', [True, False])
def test_both_aggregations_carry_jobs(hosted, monkeypatch):
    from gnndelete_amd import ops
    eng, _ = _engine(hosted)
    seen, real = [], ops._spmm_raw

    def probe(*a, host=None, **k):
        if a[3].shape[1] == 64:                                    # the two layer-2 aggregations (64 floats wide)
            seen.append(None if host is None else (host[2] > 0, host[14] > 0))
        return real(*a, host=host, **k)
    monkeypatch.setattr(ops, '_spmm_raw', probe)
    eng.step()
    torch.cuda.synchronize()
    assert seen == ([(True, False), (False, True)] if hosted else [None, None])        # job 1 forward, job 2 + finalize transposed
