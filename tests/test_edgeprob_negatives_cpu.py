"""graph_utils.negative_sampling_cached (the fused edge-probability step's per-epoch draw) returns exactly what
negative_sampling returns for the same generator state, without the per-call torch.unique; and the flag that selects
the fused step parses and defaults off."""
import pytest
import torch

from gnndelete_amd.framework import graph_utils as GU
from gnndelete_amd.framework.training_args import build_parser
from helpers import random_graph


def _dense_small():
    """n = 12 with 110 of the 132 off-diagonal pairs taken: most candidates are rejected, the retry loop runs again."""
    g = torch.Generator().manual_seed(4)
    keys = torch.tensor([a * 12 + b for a in range(12) for b in range(12) if a != b])
    keys = keys[torch.randperm(keys.numel(), generator=g)[:110]]
    return torch.stack([keys // 12, keys % 12]), 12


CASES = {
    'sparse': lambda: (random_graph(500, 3000, 1), 500),
    'dense_n12': _dense_small,
    'isolated_tail': lambda: (random_graph(300, 900, 2, isolate=40), 300),
}


@pytest.mark.parametrize('want', [1, 17, 40])
@pytest.mark.parametrize('case', sorted(CASES))
def test_cached_sampler_equals_negative_sampling(case, want, monkeypatch):
    ei, n = CASES[case]()
    keys = GU.positive_edge_keys(ei, n)
    assert torch.equal(keys, torch.unique(ei[0] * n + ei[1]))
    calls = []
    real_randint = torch.randint

    def counting(*a, **k):
        calls.append(a[2])
        return real_randint(*a, **k)
    monkeypatch.setattr(torch, 'randint', counting)
    torch.manual_seed(1234)
    ref = [GU.negative_sampling(edge_index=ei, num_nodes=n, num_neg_samples=want) for _ in range(3)]
    ref_calls, calls[:] = list(calls), []
    torch.manual_seed(1234)
    got = [GU.negative_sampling_cached(keys, n, want) for _ in range(3)]
    assert calls == ref_calls                                    # the same randint calls with the same candidate counts
    for a, b in zip(ref, got):
        assert a.dtype == b.dtype and a.shape == (2, want) and torch.equal(a, b)
    if case == 'dense_n12' and want > 1:
        assert len(ref_calls) > 3                                # some draw went round the retry loop more than once
    pos = set(keys.tolist())
    for b in got:
        assert not (set((b[0] * n + b[1]).tolist()) & pos) and bool((b[0] != b[1]).all())
    # an explicit generator takes the same path
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    assert torch.equal(GU.negative_sampling(ei, n, want, generator=g1), GU.negative_sampling_cached(keys, n, want, generator=g2))


def test_fused_edgeprob_flag_parses_and_defaults_off():
    assert build_parser().parse_args([]).fused_edgeprob is False
    assert build_parser().parse_args(['--unlearning_model', 'gnndelete', '--fused_edgeprob']).fused_edgeprob is True

