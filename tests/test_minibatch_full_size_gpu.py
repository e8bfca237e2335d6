"""GraphSAINT mini-batch unlearning at the size the fused batch step is measured at (synth-collab, 8,192 walk roots, walk
length 2, 128 -> 128 -> 64; tools/experiments/minibatch_fused.py) against the float64 oracle - not against another HIP path.

  * teacher-forced batches: per batch, the gradients the step hands to Adam (W_D1 from loss1 plus the carried loss2
    gradient, W_D2 from loss2), the W_D1 gradient it carries into the next batch and its four squared-difference sums,
    each against oracle.gnndelete_ref in float64 on the same batch (pyg_semantics.saint_subgraph) from the HIP weights
    just before it - GCN and GAT on the fused step, GraphSAGE (config 3's model) on the autograd loop it falls back to;
    the first sampled batches plus a batch without a Df edge and one without an S1 row;
  * the free-running trajectory: one epoch of NUM_STEPS injected batches, per-step losses and final Del weights against
    nodeemb_minibatch in float64 (a child process, tests/oracle_jobs.py, while this process uses the GPU).

Bounds (fixed before any result was looked at): HIP's distance to float64 <= 2 x the largest distance of an fp32 ensemble
(the same oracle in fp32 with other edge orders inside each batch), never below 5e-5 (helpers.assert_del_weights_within_
fp32_spread); the per-batch gradients, sums and per-step losses in addition under a hard ceiling of 1e-4."""
import functools
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import oracle_jobs
from helpers import assert_del_weights_within_fp32_spread, hip_model, rel_l2

pytestmark = pytest.mark.gpu
NUM_STEPS = 16                  # = oracle_jobs.JOBS['minibatch-collab-*'] num_steps
TEACHER = 4                     # teacher-forced sampled batches (+ the two edge-case batches)
CEIL = 1e-4
JOBS = ('minibatch-collab-gcn', 'minibatch-collab-gat')


def _start_jobs():
    for name in JOBS:
        assert oracle_jobs.JOBS[name][1]['num_steps'] == NUM_STEPS
        oracle_jobs.start(name)


@functools.lru_cache(maxsize=1)
def _request(gnn):
    return oracle_jobs.minibatch_request(gnn, NUM_STEPS)


def _within(tag, name, d_hip, d_ens, ceiling=CEIL):
    print(f'[{tag}] {name}: distance to fp64: fp32 ensemble ' + ' '.join(f'{v:.2e}' for v in d_ens) + f' / HIP {d_hip:.2e}'
          + f' (bound {min(max(2.0 * max(d_ens), 5e-5), ceiling):.2e})')
    assert d_hip <= max(2.0 * max(d_ens), 5e-5), (tag, name, d_hip, d_ens)
    assert d_hip <= ceiling, (tag, name, d_hip)


def _batch_reference(gnn, state, w1, w2, data, nodes, neg, dtype, perm=None):
    """oracle.gnndelete_ref on one batch in `dtype` (CPU) from Del weights (w1, w2): -> dict of dL1/dW_D1, dL2/dW_D1,
    dL2/dW_D2 (float64) and the four squared-difference sums (DEC 1, NI 1, DEC 2, NI 2).  perm: the batch's edge
    columns permuted before message passing (an fp32 ensemble member)."""
    from oracle import gnndelete_ref as R
    from oracle import pyg_semantics as pyg
    ref = R.TwoLayerDelete(gnn, data.x.shape[1], 128, 64)
    ref.load_state_dict(state, strict=False)
    with torch.no_grad():
        ref.deletion1.deletion_weight.copy_(w1)
        ref.deletion2.deletion_weight.copy_(w2)
    ref = ref.to(dtype)
    b = pyg.saint_subgraph({k: v for k, v in data.items()}, nodes)
    pos = b['edge_index'][:, b['df_mask']]
    ei, sdf = b['edge_index'], b['sdf_mask']
    if perm is not None:
        p = torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(perm))
        ei, sdf = ei[:, p], sdf[p]
    x = b['x'].to(dtype)
    with torch.no_grad():
        z1o, z2o = ref.get_original_embeddings(x, ei, return_all_emb=True)
    z1, z2 = ref(x, ei[:, sdf], None, b['sdf_node_1hop_mask'], b['sdf_node_2hop_mask'], return_all_emb=True)
    ni1, ni2 = b['sdf_node_1hop_mask_non_df_mask'], b['sdf_node_2hop_mask_non_df_mask']
    r1, r2, l1, l2 = R.nodeemb_terms(z1, z2, z1o, z2o, pos, neg, ni1, ni2, nn.MSELoss())
    a = oracle_jobs.MB_ALPHA
    W1, W2 = ref.deletion1.deletion_weight, ref.deletion2.deletion_weight

    def grads(loss, params):
        gs = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
        return [torch.zeros_like(p_).double() if g_ is None else g_.double() for g_, p_ in zip(gs, params)]
    (g1_l1,) = grads(a * r1 + (1 - a) * l1, [W1])
    g1_l2, g2 = grads(a * r2 + (1 - a) * l2, [W1, W2])
    with torch.no_grad():
        def dec(z, zo):
            return float(((torch.cat([z[pos[0]], z[pos[1]]]) - torch.cat([zo[neg[0]], zo[neg[1]]])).double() ** 2).sum())
        sums = torch.tensor([dec(z1, z1o), float(((z1[ni1] - z1o[ni1]).double() ** 2).sum()), dec(z2, z2o),
                             float(((z2[ni2] - z2o[ni2]).double() ** 2).sum())], dtype=torch.float64)
    return dict(g1_l1=g1_l1, g1_l2=g1_l2, g2=g2, sums=sums)


def _compare_batch(tag, gnn, state, data, nodes, neg, hip, w1, w2, carry):
    """hip: dict g1_adam (handed to Adam for W_D1, carry included), g2, g1_l2, sums - against fp64 and the ensemble."""
    want = _batch_reference(gnn, state, w1, w2, data, nodes, neg, torch.float64)
    ens = [_batch_reference(gnn, state, w1, w2, data, nodes, neg, torch.float32, p) for p in oracle_jobs.MB_PERMS]
    for key, name, add in (('g1_l1', 'W_D1 gradient handed to Adam (loss1 + carried)', carry),
                           ('g2', 'W_D2 gradient (loss2)', None), ('g1_l2', 'W_D1 gradient carried (loss2)', None)):
        w_ = want[key] + add if add is not None else want[key]
        e_ = [e[key] + add if add is not None else e[key] for e in ens]
        hk = 'g1_adam' if key == 'g1_l1' else key
        _within(tag, name, rel_l2(hip[hk], w_), [rel_l2(e, w_) for e in e_])
    for k, name in enumerate(('DEC 1', 'NI 1', 'DEC 2', 'NI 2')):
        w_, h_ = float(want['sums'][k]), float(hip['sums'][k])
        if w_ == 0.0:                                      # a sum over zero terms
            assert h_ == 0.0, (tag, name, h_)
            continue
        _within(tag, f'{name} sum', abs(h_ - w_) / abs(w_), [abs(float(e['sums'][k]) - w_) / abs(w_) for e in ens])


def _batches(req):
    data, state, sets, negs, edge_sets, edge_negs = req
    labels = [f'batch {i}' for i in range(TEACHER)] + ['no Df edge', 'no S1 row']
    return list(zip(labels, sets[:TEACHER] + edge_sets, negs[:TEACHER] + edge_negs))


def _fused_step(gnn, data, state, sets):
    from gnndelete_amd.framework.trainer import sampler as S
    from gnndelete_amd.minibatch import MinibatchNodeembStep
    model = hip_model(gnn, state, data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
    loader = S.FixedNodeSets(data, sets)
    return MinibatchNodeembStep(model, data, loader, oracle_jobs.MB_ALPHA, oracle_jobs.MB_LR, (0.9, 0.999), 1e-8,
                                max_nodes=3 * 8192)


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_step_teacher_forced_batches_vs_fp64(gnn, monkeypatch):
    from gnndelete_amd.framework.trainer import sampler as S
    t0 = time.time()
    _start_jobs()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    req = _request(gnn)
    data, state, sets = req[0], req[1], req[2]
    batches = _batches(req)
    step = _fused_step(gnn, data, state, [b[1] for b in batches])
    cur = {}
    monkeypatch.setattr(S, 'negative_sampling', lambda ei, n, k: cur['neg'].to(ei.device))
    handed = []
    adam = step._adam
    step._adam = lambda k, p, grad: (handed.append(grad.detach().double().cpu()), adam(k, p, grad))
    for label, nodes, neg in batches:
        w1, w2 = step.wd1.detach().double().cpu(), step.wd2.detach().double().cpu()
        carry = step.g1.detach().double().cpu() if step.g1_live else torch.zeros_like(w1)
        handed.clear()
        cur['neg'] = neg
        sums = torch.zeros(4, device='cuda')
        step.step(nodes, sums)
        assert len(handed) == 2
        cnt = step.cut.cnt
        if label == 'no Df edge':
            assert cnt[3] == 0 and neg.shape[1] == 0
        if label == 'no S1 row':
            assert cnt[4] == 0
        hip = dict(g1_adam=handed[0], g2=handed[1], g1_l2=step.g1.detach().double().cpu(), sums=sums.double().cpu())
        _compare_batch(f'{gnn} fused, {label}: {cnt[0]} nodes, {cnt[1]} edges, {cnt[3]} Df', gnn, state, data, nodes, neg, hip,
                       w1.float(), w2.float(), carry)
    print(f'[{gnn} fused] teacher-forced batches: {time.time() - t0:.1f} s')


def test_sage_autograd_loop_teacher_forced_batches_vs_fp64(monkeypatch, tmp_path):
    """GraphSAGE has no fused step: the batches run on the autograd loop (sampler.train_minibatch), whose .grad values
    at each optimizer step are compared."""
    from gnndelete_amd.framework.trainer import sampler as S
    t0 = time.time()
    _start_jobs()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    req = _request('sage')
    data, state = req[0], req[1]
    batches = _batches(req)
    model = hip_model('sage', state, data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
    W1, W2 = model.deletion1.deletion_weight, model.deletion2.deletion_weight
    opt = [torch.optim.Adam([W1], lr=oracle_jobs.MB_LR), torch.optim.Adam([W2], lr=oracle_jobs.MB_LR)]
    rec = []

    def wrap(k):
        orig = opt[k].step

        def step(*a, **kw):
            g1 = W1.grad if W1.grad is not None else torch.zeros_like(W1)
            rec.append((k, W1.detach().double().cpu(), W2.detach().double().cpu(), g1.detach().double().cpu(),
                        W2.grad.detach().double().cpu() if k == 1 else None))
            return orig(*a, **kw)
        opt[k].step = step
    wrap(0)
    wrap(1)
    monkeypatch.setattr(S, 'make_sampler', lambda d, batch_size, num_steps, walk_length=2:
                        S.FixedNodeSets(d, [b[1] for b in batches]))
    it = iter([b[2] for b in batches])
    monkeypatch.setattr(S, 'negative_sampling', lambda ei, n, k: next(it).to(ei.device))
    args = SimpleNamespace(batch_size=8192, num_steps=len(batches), epochs=1, valid_freq=2, checkpoint_dir=str(tmp_path))
    trainer = SimpleNamespace(args=SimpleNamespace(alpha=oracle_jobs.MB_ALPHA), trainer_log={})
    S.train_minibatch(trainer, model, data, opt, args)
    assert len(rec) == 2 * len(batches)
    carry = torch.zeros(128, 128, dtype=torch.float64)
    for i, (label, nodes, neg) in enumerate(batches):
        (k0, w1, w2, g1_adam, _), (k1, _, _, g1_l2, g2) = rec[2 * i], rec[2 * i + 1]
        assert (k0, k1) == (0, 1)
        hip = dict(g1_adam=g1_adam, g2=g2, g1_l2=g1_l2, sums=None)
        want = _batch_reference('sage', state, w1.float(), w2.float(), data, nodes, neg, torch.float64)
        ens = [_batch_reference('sage', state, w1.float(), w2.float(), data, nodes, neg, torch.float32, p)
               for p in oracle_jobs.MB_PERMS]
        tag = f'sage autograd loop, {label}'
        for key, hk, name, add in (('g1_l1', 'g1_adam', 'W_D1 gradient handed to Adam (loss1 + carried)', carry),
                                   ('g2', 'g2', 'W_D2 gradient (loss2)', 0), ('g1_l2', 'g1_l2', 'W_D1 gradient carried (loss2)', 0)):
            w_ = want[key] + add
            _within(tag, name, rel_l2(hip[hk], w_), [rel_l2(e[key] + add, w_) for e in ens])
        carry = g1_l2
    print(f'[sage autograd loop] teacher-forced batches: {time.time() - t0:.1f} s')


@pytest.mark.parametrize('gnn', ['gcn', 'gat'])
def test_fused_step_free_running_epoch_vs_fp64(gnn, monkeypatch):
    from gnndelete_amd.framework.trainer import sampler as S
    from gnndelete_amd.minibatch import _step_log
    t0 = time.time()
    _start_jobs()
    data, state, sets, negs, _, _ = _request(gnn)
    step = _fused_step(gnn, data, state, sets)
    it = iter(negs)
    monkeypatch.setattr(S, 'negative_sampling', lambda ei, n, k: next(it).to(ei.device))
    hist = torch.zeros(NUM_STEPS, 4, device='cuda')
    divs = [step.step(nodes, hist[i]) for i, nodes in enumerate(sets)]
    logs = [_step_log(0, s4, div, oracle_jobs.MB_ALPHA) for s4, div in zip(hist.tolist(), divs)]
    w_hip = (step.wd1.detach().double().cpu(), step.wd2.detach().double().cpu())
    t_gpu = time.time() - t0
    res = oracle_jobs.result(f'minibatch-collab-{gnn}')
    assert res['checksum'] == oracle_jobs.minibatch_checksum(state, sets, negs)
    runs = res['runs']
    r64 = runs[(str(torch.float64), None)]
    ens = [runs[(str(torch.float32), p)] for p in oracle_jobs.MB_PERMS]
    tag = f'{gnn} fused, {NUM_STEPS}-step epoch'
    for key in ('train_loss', 'train_loss_l', 'train_loss_r'):
        want = np.array([s_[key] for s_ in r64['logs']])
        assert np.isfinite(want).all()

        def dist(logs_):
            return float(np.max(np.abs(np.array([s_[key] for s_ in logs_]) - want) / np.abs(want)))
        _within(tag, f'per-step {key} (max relative)', dist(logs), [dist(e['logs']) for e in ens])
    assert_del_weights_within_fp32_spread(tag, w_hip, (r64['w1'], r64['w2']), [(e['w1'], e['w2']) for e in ens], NUM_STEPS)
    print(f'[{tag}] wall {time.time() - t0:.1f} s (HIP leg {t_gpu:.1f} s)')
