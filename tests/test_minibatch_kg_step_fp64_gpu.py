"""The fused knowledge-graph batch step (gnndelete_amd.minibatch.MinibatchKGNodeembStep) on batches past one 1,024-row scan
chunk against the float64 oracle - test_minibatch_full_size_gpu.py::test_fused_step_teacher_forced_batches_vs_fp64 for the
typed path, at the smallest size that crosses the chunks (4,000 nodes, 900 walk roots: about 1,840 nodes and 30,000 Dr edges
per batch).

Per batch, in one step object so that the carried W_D1 gradient is exercised: the gradient the step hands to Adam for W_D1
(loss 1 plus what loss 2 left last batch), the W_D2 gradient, the W_D1 gradient it leaves in step.g1 and its four
squared-difference sums, each against oracle.gnndelete_ref.TwoLayerDelete('rgcn') in float64 on pyg_semantics.saint_subgraph
of the same nodes from the HIP Del weights just before the batch (kg_batch_cases.step_batch_reference, computed inline on the
host).  Negatives are recorded ones (the oracle's negative_sampling_kg under a seeded generator on the oracle's decoded
triples), fed through framework.utils.negative_sampling_kg, which step() looks up at call time.

Bound: test_minibatch_full_size_gpu.py::_within, unchanged - HIP's distance to float64 <= 2 x the largest distance of the
fp32 ensemble (the same oracle in fp32 with edge orders None, 1, 2), never below 5e-5, under a hard ceiling of 1e-4.  The
ensemble is measured here from the reference alone; test_kg_batch_cases_cpu.py shows it at 2e-7 .. 4e-7, so the floor is the
bound.  Both distances are printed per batch and quantity."""
import time

import pytest
import torch

import kg_batch_cases as K
from helpers import hip_model
from test_minibatch_full_size_gpu import _within

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('config', sorted(K.STEP_CONFIGS))
def test_fused_kg_step_teacher_forced_batches_vs_fp64(config, monkeypatch):
    from gnndelete_amd.framework import utils as U
    from gnndelete_amd.framework.trainer import sampler as S
    from gnndelete_amd.minibatch import MinibatchKGNodeembStep
    t0 = time.time()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    data, nr, dims, state, batches = K.step_request(config)
    model = hip_model('rgcn', state, data.sdf_node_1hop_mask, data.sdf_node_2hop_mask, num_nodes=int(data.num_nodes), num_edge_type=nr)
    assert (model.conv1.num_blocks == 4) == (config == 'blocks-25') and (model.conv1.num_blocks is None) == (config == 'dense-6')
    loader = S.FixedNodeSets(data, [b[1] for b in batches])
    step = MinibatchKGNodeembStep(model, data, loader, nr, K.STEP_ALPHA, 'mean', K.STEP_LR, (0.9, 0.999), 1e-8,
                                  max_nodes=3 * K.STEP_ROOTS)
    cur = {}

    def recorded_negatives(edge_index, edge_type):
        assert torch.equal(edge_index.cpu(), cur['dec']) and torch.equal(edge_type.cpu(), cur['dec_type'])      # the oracle's triples
        return cur['neg'].to(edge_index.device)
    monkeypatch.setattr(U, 'negative_sampling_kg', recorded_negatives)
    handed = []
    adam = step._adam
    step._adam = lambda k, p, grad: (handed.append(grad.detach().double().cpu()), adam(k, p, grad))
    single_reads = 0
    for i, (label, nodes, dec, dec_type, neg) in enumerate(batches):
        w1, w2 = step.wd1.detach().double().cpu(), step.wd2.detach().double().cpu()
        carry = step.g1.detach().double().cpu() if step.g1_live else torch.zeros_like(w1)
        assert step.g1_live == (i > 0)
        handed.clear()
        cur.update(dec=dec, dec_type=dec_type, neg=neg)
        sums = torch.zeros(4, device='cuda')
        reads, e_cap = step.cut.reads, step.cut.e_cap
        step.step(nodes, sums)
        assert len(handed) == 2
        # one blocking host read per batch; the grow-and-recut of a batch larger than the edge buffers costs one more
        grew = step.cut.e_cap > e_cap
        assert step.cut.reads - reads == (2 if grew else 1), (label, step.cut.reads - reads, grew)
        assert grew == (i == 0)
        single_reads += not grew
        hip = dict(g1_l1=handed[0], g2=handed[1], g1_l2=step.g1.detach().double().cpu(), sums=sums.double().cpu())
        want = K.step_batch_reference(config, w1.float(), w2.float(), nodes, neg, torch.float64)
        ens = [K.step_batch_reference(config, w1.float(), w2.float(), nodes, neg, torch.float32, p) for p in K.STEP_PERMS]
        cnt = step.cut.cnt
        assert tuple(cnt[:5]) == want['counts'] and cnt[5] == 0
        if label == 'no decoded Df triple':
            assert cnt[2] == 0 and neg.shape[1] == 0
        if label == 'no list-1 row':
            assert cnt[3] == 0
        tag = f'rgcn {config} fused, {label}: {cnt[0]} nodes, {cnt[1]} Dr edges, {cnt[2]} decoded'
        d_hip = K.step_distances(hip, want, carry, got_holds_carry=True)
        d_ens = [K.step_distances(e, want, carry) for e in ens]
        for name, v in d_hip.items():
            _within(tag, name, v, [d[name] for d in d_ens])
        for k, name in enumerate(K.STEP_SUMS):
            if float(want['sums'][k]) == 0.0:              # a sum over zero terms
                assert float(hip['sums'][k]) == 0.0, (tag, name, float(hip['sums'][k]))
        assert len(d_hip) == 7 - int((want['sums'] == 0.0).sum())
    assert single_reads == len(batches) - 1
    print(f'[rgcn {config} fused] teacher-forced batches: {time.time() - t0:.1f} s')
