"""The CPU side of tests/test_engine_large_forms_gpu.py: the shared request really sits where the engine changes kernels
(test_request_conditions), the flags written by hand in that module's case table are what engine.plan_step chooses for them,
and the table reaches EVERY fused-Del-1 form plan_step can choose at this size (test_cases_reach_every_fused_del1_form) - the
enumeration is backbone x cache_layer1 x affected_rows_only x {default knobs, every single flip of a Boolean knob that is not
R-GCN's or GraphSAGE's root term}, both_layerwise / mse; a (mode, StepForms) pair counts once, `gat_dots` only for GAT.

A dead clause this enumeration shows: plan_step's `fuse_del1` admits loss_type 'only1', but it also requires `tail`, and `tail`
requires a both_* loss type - so `fuse_del1` can never hold for 'only1'.  The behaviour is left as it is;
the clause is only noted here."""
import itertools

import torch

from gnndelete_amd.engine import Knobs, StepFacts, plan_step
from test_engine_large_forms_gpu import CASES, FLAGS, OPTS, WS_MIN_ROWS, knob_field, large_request, plain_sibling

MODES = ('gcn', 'gin', 'gat', 'sage')
FAMILY = {'mse_mean': 'mse', 'kld_mean': 'kld', 'cosine_mean': 'cosine', 'cosine_sum': 'cosine'}
# the Boolean knobs of the enumeration: all but R-GCN's and GraphSAGE's root term (`pad_out` is not Boolean)
FLIPS = [name for name, default in Knobs._field_defaults.items()
         if isinstance(default, bool) and not name.startswith('rgcn_') and name != 'sage_root_in_spmm']


def _loss_rows(layer):
    data, _, ni1, ni2 = large_request()
    rows = torch.zeros(data.num_nodes, dtype=torch.bool)
    rows[data.train_pos_edge_index[:, data.df_mask].flatten()] = True
    return rows | (ni1, ni2)[layer - 1]


def facts_for(mode, cache, rows, loss_type='both_layerwise', family='mse'):
    """StepFacts as NodeembEngine computes them for this request at 128 -> 128 -> 64 (del1_covers: s1 >= 65,536 at h = 128)."""
    data = large_request()[0]
    s1, s2 = int(data.sdf_node_1hop_mask.sum()), int(data.sdf_node_2hop_mask.sum())
    return StepFacts(mode=mode, loss_type=loss_type, family=family, h=128, o=64, s1=s1, s2=s2,
                     folded1=True, n_rows1=int(_loss_rows(1).sum()), inside1=True,
                     folded2=True, n_rows2=int(_loss_rows(2).sum()), inside2=True,
                     cache_layer1=cache, rows_only_asked=rows, closed=rows, w2_mfma=True, gin_ok=mode == 'gin',
                     del1_covers=True, pair_covers=True)


def case_plan(case):
    opts = OPTS[case.opts]
    facts = facts_for(case.gnn, bool(opts.get('cache_layer1')), bool(opts.get('affected_rows_only')), case.loss_type,
                      FAMILY[case.loss_fct])
    knobs = Knobs() if case.knob is None else Knobs()._replace(**dict([knob_field(case)]))
    return plan_step(facts, knobs)


def _key(mode, forms):
    return mode, (forms if mode == 'gat' else forms._replace(gat_dots=True))


def test_request_conditions():
    """The conditions the GPU module's cases rely on - not the values: a request that drifts with the generator still has to sit
    above the threshold, end in partial 64-row units, be closed under the graph and have rows longer than one wave."""
    data, neg, ni1, ni2 = large_request()
    n = data.num_nodes
    m1, m2 = data.sdf_node_1hop_mask, data.sdf_node_2hop_mask
    s1, s2 = int(m1.sum()), int(m2.sum())
    E = data.train_pos_edge_index
    e_sdf, pos = E[:, data.sdf_mask], E[:, data.df_mask]
    deg = torch.bincount(e_sdf[1], minlength=n)
    print(f'n = {n}, s1 = {s1} (= {s1 % 64} mod 64), s2 = {s2} (= {s2 % 64} mod 64), Df columns {pos.shape[1]}, S_Df edges '
          f'{e_sdf.shape[1]}, max degree {int(deg.max())}, isolated nodes {int((torch.bincount(E.flatten(), minlength=n) == 0).sum())}')
    assert WS_MIN_ROWS <= s1 < s2 < n
    assert s1 % 64 != 0 and s2 % 64 != 0, 'the last 64-row unit of both Del passes is partial'
    assert bool(m2[e_sdf].all()), 'no S_Df edge leaves S2: the affected rows are closed under the training graph'
    assert bool((m1 <= m2).all())
    assert neg.shape == pos.shape
    assert bool(_loss_rows(1)[~m1].sum() == 0) and bool(_loss_rows(2)[~m2].sum() == 0), 'every loss row of layer k lies in S_k'
    assert not bool(ni1[pos.flatten()].any()) and not bool(ni2[pos.flatten()].any()), 'one kind of loss term per row'
    assert int(deg.max()) > 64, 'some row is longer than one wave'


def test_case_flags_are_what_plan_step_chooses():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for case in CASES:
        forms = case_plan(case)
        assert {f: getattr(forms, f) for f in FLAGS} == case.flags, (case.name, forms)
        if case.opts != 'plain' or case.knob is not None or case.graph:
            # (e) compares a variant with its plain sibling; groups B and the cosine_mean case have none, by the table's design
            assert plain_sibling(case) is not None or case.name[0] in 'BC', case.name


def test_cases_reach_every_fused_del1_form():
    reached = {_key(c.gnn, case_plan(c)) for c in CASES}
    settings = [Knobs()] + [Knobs()._replace(**{name: not Knobs._field_defaults[name]}) for name in FLIPS]
    fused, unfused = {}, {}
    for mode, cache, rows, k in itertools.product(MODES, (False, True), (False, True), settings):
        forms = plan_step(facts_for(mode, cache, rows), k)
        (fused if forms.fuse_del1 else unfused).setdefault(_key(mode, forms), (mode, cache, rows, k))
    print(f'{len(fused)} distinct (mode, forms) with fuse_del1 on, {len({f for _, f in fused})} distinct forms; '
          f'without fuse_del1: {len(unfused)}, of which the case table reaches {len(set(unfused) & reached)}')
    for key, (mode, cache, rows, k) in unfused.items():
        changed = {n_: v for n_, v in k._asdict().items() if v != Knobs._field_defaults[n_]}
        print(f'  without fuse_del1, {"reached" if key in reached else "not reached"}: {mode} cache={cache} rows={rows} {changed}')
    missing = [fused[key] for key in fused if key not in reached]
    assert not missing, missing
    assert len(fused) >= 16

