#!/usr/bin/env python3
"""Generate tests/golden/orig_nodecls_{gcn,gat,gcn_c3}.npz from the REAL reference code: the original node classifier's
training loop NodeClassificationTrainer.train (framework/trainer/base.py:694-752: log_softmax, NLL on train_mask, Adam) with
its evaluation (NodeClassificationTrainer.eval, :754-790: accuracy / micro-F1 on val_mask) on the reference's own GCN and GAT
(framework/models/{gcn,gat}.py), under the stubs and helpers of make_golden.py (imported, not copied; see its docstring for
how the reference is imported in place).  Runs only where the reference is checked out; the outputs hold data only (initial
state, the request, final state, the recorded series) and their shapes go into MANIFEST_nodecls.json.

Usage:  python tests/golden/make_golden_nodecls_orig.py"""
import importlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402

CASES = [('gcn', 'gcn', 4), ('gat', 'gat', 4), ('gcn_c3', 'gcn', 3)]      # (fixture tag, model, classes)


def nodecls_request(classes, seed):
    """~100 nodes as golden_nodecls_trajectory builds them: undirected random graph, labels, a 60 / 20 / 20 split."""
    g = G.synth_graph(100, 380, 10, seed=seed)
    n = g['num_nodes']
    gen = torch.Generator().manual_seed(seed + 1)
    E = g['train']
    und, _ = G.pyg.to_undirected(E, [torch.ones(E.shape[1], dtype=torch.int32)], n)
    y = torch.randint(0, classes, (n,), generator=gen)
    perm = torch.randperm(n, generator=gen)
    tr, va, te = (torch.zeros(n, dtype=torch.bool) for _ in range(3))
    tr[perm[:60]] = True
    va[perm[60:80]] = True
    te[perm[80:]] = True
    return G.Bag(x=g['x'], num_nodes=n, edge_index=und, y=y, train_mask=tr, val_mask=va, test_mask=te)


def golden_nodecls_original(B, A):
    models = {'gcn': importlib.import_module('framework.models.gcn').GCN,
              'gat': importlib.import_module('framework.models.gat').GAT}
    shapes = {}
    for k, (tag, gnn, classes) in enumerate(CASES):
        d = nodecls_request(classes, seed=37 + 2 * k)
        args = G.make_args(A, ['--gnn', gnn, '--unlearning_model', 'original_node', '--in_dim', '10', '--hidden_dim', '32',
                               '--out_dim', str(classes), '--dataset', 'DBLP', '--checkpoint_dir', tempfile.mkdtemp(),
                               '--lr', '0.01'])
        args.epochs, args.valid_freq = 6, 3
        torch.manual_seed(14 + k)
        model = models[gnn](args)
        with torch.no_grad():                      # non-trivial biases
            for n_, p in model.named_parameters():
                if n_.endswith('bias'):
                    p.copy_(torch.randn_like(p) * 0.1)
        init = G.state_np(model)
        model.to = lambda *a, **kw: model
        opt = torch.optim.Adam(model.parameters(), lr=args.lr)
        G.STATE['wandb'] = []
        B.NodeClassificationTrainer(args).train(model, d, opt, args)
        steps = [w for w in G.STATE['wandb'] if 'train_loss' in w]
        vals = [w for w in G.STATE['wandb'] if 'val_loss' in w]
        assert [s['epoch'] for s in steps] == [2, 5] and len(vals) == 2
        out = dict(init)
        out.update({f'd::{key}': G.np_(v) for key, v in d.items() if torch.is_tensor(v)})
        out['d::num_nodes'] = np.int64(d['num_nodes'])
        out.update({f'final::{key}': G.np_(v) for key, v in model.state_dict().items()})
        out.update(train_loss=np.array([s['train_loss'] for s in steps]), val_loss=np.array([v['val_loss'] for v in vals]),
                   val_dt_acc=np.array([v['val_dt_acc'] for v in vals]), val_dt_f1=np.array([v['val_dt_f1'] for v in vals]),
                   lr=np.float64(args.lr), epochs=np.int64(6), valid_freq=np.int64(3), classes=np.int64(classes))
        name = f'orig_nodecls_{tag}.npz'
        np.savez_compressed(os.path.join(HERE, name), **out)
        shapes[name] = {key: list(np.asarray(v).shape) for key, v in sorted(out.items())}
    with open(os.path.join(HERE, 'MANIFEST_nodecls.json'), 'w') as f:
        json.dump(shapes, f, indent=1, sort_keys=True)
        f.write('\n')


def main():
    if not os.path.isdir(G.REF):
        print('reference checkout not found:', G.REF)
        return
    D, T, TE, A, U, B = G.load_reference()
    golden_nodecls_original(B, A)
    print('node-classification training vectors written to', HERE)


if __name__ == '__main__':
    main()
