"""Shared helpers for the test-suite (fixture loading, oracle model construction)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    return {k: z[k] for k in z.files}


def t(a):
    return torch.from_numpy(np.asarray(a))


def split_fixture(fx):
    """-> (state_dict, data dict of tensors, everything else)."""
    state = {k[3:]: t(v) for k, v in fx.items() if k.startswith('w::')}
    data = {k[3:]: (int(v) if k == 'd::num_nodes' else t(v)) for k, v in fx.items() if k.startswith('d::')}
    rest = {k: v for k, v in fx.items() if '::' not in k}
    return state, data, rest


def dims_from_state(gnn, state):
    if gnn == 'gcn':
        w1, w2 = state['conv1.lin.weight'], state['conv2.lin.weight']
    elif gnn == 'gat':
        w1, w2 = state['conv1.lin_src.weight'], state['conv2.lin_src.weight']
    elif gnn == 'gin':
        w1, w2 = state['conv1.nn.weight'], state['conv2.nn.weight']
    elif gnn == 'sage':
        w1, w2 = state['conv1.lin_l.weight'], state['conv2.lin_l.weight']
    elif gnn == 'rgat':
        e, q1, q2 = state['node_emb.weight'], state['conv1.q'], state['conv2.q']
        return e.shape[1], q1.shape[0], q2.shape[0]
    else:
        r1, r2 = state['conv1.root'], state['conv2.root']
        return r1.shape[0], r1.shape[1], r2.shape[1]
    return w1.shape[1], w1.shape[0], w2.shape[0]


def oracle_model(gnn, state, mask1=None, mask2=None, num_nodes=None, num_edge_type=None, **kw):
    from oracle import gnndelete_ref as R
    i, h, o = dims_from_state(gnn, state)
    m = R.TwoLayerDelete(gnn, i, h, o, mask1, mask2, num_nodes=num_nodes, num_edge_type=num_edge_type, **kw)
    missing = m.load_state_dict(state, strict=False)
    assert not [k for k in missing.missing_keys if 'lin_dst' not in k], missing
    return m


def rel_l2(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def random_graph(n, m, seed, loops=True, dups=True, isolate=0):
    """Random directed edge list with optional self loops / multi-edges / isolated nodes."""
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, max(1, n - isolate), (2, m), generator=g)
    if not loops:
        ei = ei[:, ei[0] != ei[1]]
    if dups and ei.shape[1] > 8:
        ei = torch.cat([ei, ei[:, :8]], 1)
    return ei


def hip_model(gnn, state, mask1=None, mask2=None, num_nodes=None, num_edge_type=None, device='cuda'):
    from types import SimpleNamespace
    from gnndelete_amd.framework import models as M
    i, h, o = dims_from_state(gnn, state)
    args = SimpleNamespace(in_dim=i, hidden_dim=h, out_dim=o)
    cls = {'gcn': M.GCNDelete, 'gat': M.GATDelete, 'gin': M.GINDelete, 'rgcn': M.RGCNDelete, 'sage': M.SAGEDelete,
           'rgat': M.RGATDelete}[gnn]
    if gnn in ('rgcn', 'rgat'):
        m = cls(args, num_nodes, num_edge_type, mask1, mask2)
    else:
        m = cls(args, mask1, mask2)
    res = m.load_state_dict(state, strict=False)
    assert not res.unexpected_keys and not [k for k in res.missing_keys if 'lin_dst' not in k], res
    return m.to(device)


def free_port():
    """A TCP port that is free right now (bind to port 0): torch.distributed.run rendezvous of the multi-process tests -
    a hard-coded port collides with a concurrent run or with a socket still in TIME_WAIT."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def oracle_runner(gnn, data, state, neg, ni1, ni2, dtype, device, loss_type='both_layerwise', alpha=0.5, lr=1e-3, perm=None,
                  hidden=128, out=64, edges=None, edge_type=None, pos=None, num_edge_type=None, del_masks=None, train_mask=None,
                  loss_fct='mse_mean'):
    """The oracle (oracle/gnndelete_ref.py) as plain torch ops in `dtype` on `device`, one Del-training request:
    -> (step(), snapshot(), (z1_ori, z2_ori)).  perm = a seed: the edge lists are permuted first - a different summation order
    in every scatter, i.e. ANOTHER correct implementation of the same arithmetic (the members of an fp32 ensemble).
    step() runs one iteration and returns the oracle's log of it (train_loss, loss_r, loss_l).
    snapshot() = (W_D1, W_D2, z1 on the 1-hop S_Df nodes, z2 on the 2-hop S_Df nodes, z2) with the embeddings taken on the
    retained edges (evaluation semantics, framework/trainer/base.py:238-242); the first four as fp64 CPU tensors.
    edges / edge_type / pos override the link-prediction defaults (data.train_pos_edge_index, no types, the Df columns):
    the knowledge-graph request trains on data.edge_index with data.edge_type and decodes data.kg_dec_edge
    (gnndelete_nodeemb.py:745-800; del_masks = the masks its Del operators were built with, train_mask = data.dr_mask: that
    trainer's forward runs on the retained edges, not on S_Df), the node-deletion request on
    the undirected data.edge_index (:498-657).  loss_fct: a key of the oracle's LOSSES (the KLD / cosine families)."""
    from oracle import gnndelete_ref as R
    # (the GPU box has 256 host threads: the oracle's small host-side tensor ops are ~6 x slower with all of them than with 32)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    m1, m2 = del_masks if del_masks is not None else (data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
    relational = gnn in ('rgcn', 'rgat')
    E = data.train_pos_edge_index if edges is None else edges
    if pos is None:
        pos = E[:, data.df_mask]
    tm = data.sdf_mask if train_mask is None else train_mask
    e_dr, e_sdf = E[:, data.dr_mask], E[:, tm]
    t_dr, t_sdf = (edge_type[data.dr_mask], edge_type[tm]) if relational else (None, None)
    if relational:
        ref = R.TwoLayerDelete(gnn, hidden, hidden, out, m1, m2, num_nodes=data.num_nodes, num_edge_type=num_edge_type)
    else:
        ref = R.TwoLayerDelete(gnn, data.x.shape[1], hidden, out, m1, m2)
    ref.load_state_dict(state, strict=False)
    ref = ref.to(dtype).to(device)
    x = (data.x if relational else data.x.to(dtype)).to(device)
    ed, es = e_dr.to(device), e_sdf.to(device)
    if relational:
        t_dr, t_sdf = t_dr.to(device), t_sdf.to(device)
    if perm is not None:
        gp = torch.Generator().manual_seed(perm)
        pd, ps = torch.randperm(ed.shape[1], generator=gp).to(device), torch.randperm(es.shape[1], generator=gp).to(device)
        ed, es = ed[:, pd], es[:, ps]
        if relational:
            t_dr, t_sdf = t_dr[pd], t_sdf[ps]
    with torch.no_grad():
        z1o, z2o = ref.get_original_embeddings(x, ed, t_dr, return_all_emb=True)
    tg = dict(z1_ori=z1o, z2_ori=z2o, pos_edge=pos.to(device), neg_edge=neg.to(device), ni_mask1=ni1.to(device),
              ni_mask2=ni2.to(device))
    opt = R.make_optimizer(ref, loss_type, lr)
    def step():
        log = R.nodeemb_epoch(ref, lambda: ref(x, es, t_sdf, return_all_emb=True), tg, opt, loss_type, alpha, R.LOSSES[loss_fct])
        return {k: log[k] for k in ('train_loss', 'loss_r', 'loss_l')}

    def snapshot():
        with torch.no_grad():
            z1, z2 = ref(x, ed, t_dr, return_all_emb=True)
        return (ref.deletion1.deletion_weight.detach().double().cpu(), ref.deletion2.deletion_weight.detach().double().cpu(),
                z1[m1.to(device)].double().cpu(), z2[m2.to(device)].double().cpu(), z2.detach())
    return step, snapshot, (z1o, z2o)


def assert_del_weights_within_fp32_spread(tag, hip_w, w64, ens, iters):
    """The Del WEIGHTS are a looser observable than the embeddings north_star bounds: Adam's first updates are
    lr * m / sqrt(v) ~ +-lr per entry whatever the gradient's size, so the fp32 summation-order noise of a 180k-row
    weight-gradient reduction shows up undamped in the weight, while the embeddings see it scaled by lr.  So they are held
    to what fp32 arithmetic itself can deliver: HIP's distance to the fp64 oracle's weights <= 2 x the largest distance of
    an fp32 ENSEMBLE (the same oracle in fp32 with several scatter orders; for the CPU-sized cases also the CPU oracle) to them
    (+ 5e-5: the ensemble's own spread from run to run is a factor of four at this horizon - 3.5e-6 ... 1.4e-5 for W_D1 of
    GCN at collab size - while HIP sits at 1.5e-5 every time; 5e-5 is 20 x below the 1e-3 this assertion replaced)."""
    for k, name in enumerate(('W_D1', 'W_D2')):
        d_ens = [rel_l2(e[k], w64[k]) for e in ens]
        d_hip = rel_l2(hip_w[k], w64[k])
        print(f'[{tag}] {name} after {iters} iterations, rel-L2 to the fp64 oracle: fp32 ensemble '
              + ' '.join(f'{v:.2e}' for v in d_ens) + f' / HIP {d_hip:.2e}')
        assert d_hip <= max(2.0 * max(d_ens), 5e-5), (name, d_hip, d_ens)
