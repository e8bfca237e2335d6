"""Base trainers: original link-prediction / node-classification training, evaluation, logs,
checkpoints.  Mirrors the public surface of the reference's framework/trainer/base.py
(Trainer :24-392, NodeClassificationTrainer :694-864): same method names and signatures, same
trainer_log / checkpoint / file formats, same evaluation protocol including its quirks
(BCE-with-logits on already-sigmoided scores :243-247; Df labelled 0 and Dr labelled 1
:274-277; 500 cached random Dr subsets :263-268; `test` stage of the node classifier reading
val_mask :768-771).  All model arithmetic runs on the HIP kernels; AUC / AUP / accuracy stay
on the host with scikit-learn exactly as upstream."""
import json
import os
import time

import numpy as np
import torch
import torch.nn.functional as F
from sklearn.metrics import accuracy_score, f1_score

from ..evaluation import verification_error
from ..graph_utils import negative_sampling
from ...rankeval import fused_eval_unsupported, subset_auc_ap      # (--fused_eval; imports numpy and torch only)
from ..metrics import batched_average_precision, batched_roc_auc
from ..training_args import is_large
from ..utils import get_link_labels
from ._log import fmt, wandb_log

device = torch.device('cuda') if torch.cuda.is_available() else torch.device('cpu')


def _all_pairs(z):
    """z z^T on the host, as Trainer.eval(pred_all=True) hands it to test() / save_log (framework/trainer/base.py:288 upstream);
    the product runs on the HIP dense kernels (ops.gram), not on torch's matmul."""
    from ... import ops
    return ops.gram(z.detach()).cpu()


def _require_gpu():
    if not torch.cuda.is_available():
        from ... import _lib
        raise _lib.GnnDeleteHipError('training/evaluation runs on the HIP kernels: a GPU is required (no CPU fallback)')


class Trainer:
    def __init__(self, args):
        self.args = args
        self.trainer_log = {'unlearning_model': args.unlearning_model, 'dataset': args.dataset, 'log': []}
        self.logit_all_pair = None
        self.df_pos_edge = []
        os.makedirs(self.args.checkpoint_dir, exist_ok=True)
        with open(os.path.join(self.args.checkpoint_dir, 'training_args.json'), 'w') as f:
            json.dump(vars(args), f)

    # ------------------------------------------------------------------ helpers
    @torch.no_grad()
    def get_link_labels(self, pos_edge_index, neg_edge_index):
        return get_link_labels(pos_edge_index, neg_edge_index)

    @torch.no_grad()
    def get_embedding(self, model, data, on_cpu=False):
        return model(data.x, data.train_pos_edge_index[:, data.dtrain_mask])

    def _record(self, *records, keep=True):
        for rec in records:
            wandb_log(rec)
            print(fmt(rec))
            if keep:
                self.trainer_log['log'].append(rec)

    # ------------------------------------------------------------------ original training
    def train(self, model, data, optimizer, args):
        # Cora / PubMed / DBLP / CS full batch; the reference's mini-batch branch (ogbl-*, Physics) exists to fit a
        # 16-32 GB GPU - one MI355X holds these graphs whole, so it is taken only on request (--minibatch)
        if is_large(self.args.dataset) and getattr(args, 'minibatch', False):
            self._fused_backbone_applies(model, optimizer, args)        # (--fused_backbone: leaves its reason in the log)
            return self.train_minibatch(model, data, optimizer, args)
        return self.train_fullbatch(model, data, optimizer, args)

    # ------------------------------------------------------------------ --fused_backbone (gnndelete_amd/backbone.py)
    def _fused_backbone_applies(self, model, optimizer, args, task='linkpred'):
        """Does this run take the fused backbone step?  With the flag, trainer_log['backbone_step'] says 'fused' or why not."""
        if not getattr(args, 'fused_backbone', False):
            return False
        from ...backbone import fused_backbone_unsupported
        reason = fused_backbone_unsupported(model, args, optimizer, task)
        self.trainer_log['backbone_step'] = 'fused' if reason is None else reason
        if reason is not None:
            print(f'--fused_backbone: {reason}; running the autograd loop', flush=True)
        return reason is None

    def _backbone_engine(self, model, data, edges, n_neg, optimizer, args):
        """The engine of one train call: message passing and positives on `edges`, Adam's hyper-parameters and state from the
        caller's optimizer (a second train call on the same model and optimizer continues the first)."""
        from ...backbone import BackboneEngine
        from .gnndelete_nodeemb import _adam_hyper
        lr, betas, eps = _adam_hyper(optimizer)
        engine = BackboneEngine(model, data.x, edges, edges, n_neg, lr, betas, eps, history=max(16, args.epochs))
        engine.import_adam_state(optimizer)
        self._backbone = engine
        return engine

    @staticmethod
    def _cached_negative_draw(sampler, edges, num_nodes):
        """The epoch's draw for the fused step: the same random stream as `sampler` (a trainer module's negative_sampling),
        without its torch.unique over every positive edge on every epoch; None when the module-level name has been replaced
        (the tests' seam), and the caller keeps calling it."""
        from .. import graph_utils
        if sampler is not graph_utils.negative_sampling:
            return None
        pos_keys = graph_utils.positive_edge_keys(edges, num_nodes)
        return lambda n_neg: graph_utils.negative_sampling_cached(pos_keys, num_nodes, n_neg)

    def _device_negative_keys(self, args, fused, sampler, edges, num_nodes, flag='fused_backbone'):
        """--device_negatives: the sorted keys of `edges` (the pairs the host draw excludes) when this run draws its negatives
        on the device, else None and the host draw stays; with the flag, trainer_log['negatives'] says 'device' or why not.
        fused: whether the fused step (--`flag`) applies; sampler: the trainer module's negative_sampling (the tests' seam)."""
        if not getattr(args, 'device_negatives', False):
            return None
        from ...negatives import device_negatives_fallback
        from .. import graph_utils
        replaced = sampler is not graph_utils.negative_sampling
        keys = graph_utils.positive_edge_keys(edges, num_nodes) if fused and not replaced else None
        reason = device_negatives_fallback(flag, fused, replaced, None if keys is None else keys.numel(), num_nodes)
        self.trainer_log['negatives'] = 'device' if reason is None else reason
        if reason is not None:
            print(f'--device_negatives: {reason}; drawing the negatives on the host', flush=True)
            return None
        return keys

    def train_minibatch(self, model, data, optimizer, args):
        """base.py:144-227: per GraphSAINT batch, BCE link prediction on the batch's edges against one negative per
        edge; best-validation-loss checkpoint."""
        from . import sampler as _sampler
        _require_gpu()
        if getattr(args, 'fused_minibatch', False):
            # --fused_minibatch: the same loop with each batch on the fused HIP batch step (gnndelete_amd/minibatch.py)
            from ...minibatch import fused_minibatch_backbone_unsupported, train_minibatch_backbone_fused
            reason = fused_minibatch_backbone_unsupported(model, args, optimizer)
            if reason is None:
                self.trainer_log['minibatch_step'] = 'fused'
                return train_minibatch_backbone_fused(self, model, data, optimizer, args)
            print(f'--fused_minibatch: {reason}; running the autograd mini-batch loop', flush=True)
            self.trainer_log['minibatch_step'] = 'autograd'
        start = time.time()
        best_valid_loss, best_epoch = 1000000, 0
        model = model.to(device)
        data = data.to('cpu')
        data.edge_index = data.train_pos_edge_index
        loader = _sampler.make_sampler(data, args.batch_size, args.num_steps)
        self.trainer_log['steps'] = []
        for epoch in range(args.epochs):
            model.train()
            epoch_loss, steps, z = 0.0, 0, None
            for batch in loader:
                edges = batch.edge_index.to(device).contiguous()
                z = model(batch.x.to(device), edges)
                neg = _sampler.negative_sampling(edges, z.size(0), edges.shape[1])
                loss = F.binary_cross_entropy_with_logits(model.decode(z, edges, neg), get_link_labels(edges, neg))
                loss.backward()
                optimizer.step()
                optimizer.zero_grad()
                rec = {'epoch': epoch, 'step': steps, 'train_loss': loss.item()}
                wandb_log(rec)
                self.trainer_log['steps'].append(rec)
                epoch_loss += rec['train_loss']
                steps += 1
            if (epoch + 1) % args.valid_freq == 0:
                valid_loss, *_, valid_log = self.eval(model, data, 'val')
                self._record({'epoch': epoch, 'train_loss': epoch_loss / max(steps - 1, 1)}, valid_log)
                if valid_loss < best_valid_loss:
                    best_valid_loss, best_epoch = valid_loss, epoch
                    print(f'Save best checkpoint at epoch {epoch:04d}. Valid loss = {valid_loss:.4f}')
                    torch.save({'model_state': model.state_dict(), 'optimizer_state': optimizer.state_dict()},
                               os.path.join(args.checkpoint_dir, 'model_best.pt'))
                    torch.save(z.detach(), os.path.join(args.checkpoint_dir, 'node_embeddings.pt'))
                data = data.to('cpu')
        self.trainer_log['training_time'] = time.time() - start
        torch.save({'model_state': model.state_dict(), 'optimizer_state': optimizer.state_dict()},
                   os.path.join(args.checkpoint_dir, 'model_final.pt'))
        self.trainer_log['best_epoch'], self.trainer_log['best_valid_loss'] = best_epoch, best_valid_loss

    def train_fullbatch(self, model, data, optimizer, args):
        """BCE link prediction on all train edges vs fresh negatives each epoch (base.py:75-142)."""
        _require_gpu()
        start = time.time()
        best_valid_loss, best_epoch = 1000000, 0
        model = model.to(device)
        data = data.to(device)
        edges = data.train_pos_edge_index
        n_neg = int(data.dtrain_mask.sum()) if hasattr(data, 'dtrain_mask') else edges.shape[1]
        fused = self._fused_backbone_applies(model, optimizer, args)
        engine = None
        draw = self._cached_negative_draw(negative_sampling, edges, data.num_nodes) if fused else None
        device_keys = self._device_negative_keys(args, fused, negative_sampling, edges, data.num_nodes)
        for epoch in range(args.epochs):
            model.train()
            if device_keys is not None:             # --device_negatives: no host work between the epochs' replays
                if engine is None:
                    engine = self._backbone_engine(model, data, edges.contiguous(), n_neg, optimizer, args)
                    engine.enable_device_negatives(device_keys, args.random_seed)
                engine.step_device()
            elif fused:
                neg = draw(n_neg) if draw is not None else negative_sampling(edges, data.num_nodes, n_neg)
                if engine is None:                  # (sized by the first draw: the loop takes whatever count the sampler gives)
                    engine = self._backbone_engine(model, data, edges.contiguous(), int(neg.shape[1]), optimizer, args)
                engine.step(neg)
            else:
                neg = negative_sampling(edges, data.num_nodes, n_neg)
                z = model(data.x, edges)
                logits = model.decode(z, edges, neg)
                loss = F.binary_cross_entropy_with_logits(logits, get_link_labels(edges, neg))
                loss.backward()
                optimizer.step()
                optimizer.zero_grad()
            if (epoch + 1) % args.valid_freq == 0:
                if fused:
                    train_loss, z = engine.last_loss(), engine.z.clone()    # the block's host read; z of this epoch's forward
                    engine.export_adam_state(optimizer)                     # (a checkpoint below carries the optimizer's state)
                else:
                    train_loss = loss.item()
                valid_loss, *_, valid_log = self.eval(model, data, 'val')
                self._record({'epoch': epoch, 'train_loss': train_loss}, valid_log)
                if valid_loss < best_valid_loss:
                    best_valid_loss, best_epoch = valid_loss, epoch
                    print(f'Save best checkpoint at epoch {epoch:04d}. Valid loss = {valid_loss:.4f}')
                    torch.save({'model_state': model.state_dict(), 'optimizer_state': optimizer.state_dict()},
                               os.path.join(args.checkpoint_dir, 'model_best.pt'))
                    torch.save(z.detach(), os.path.join(args.checkpoint_dir, 'node_embeddings.pt'))
        if engine is not None:
            engine.export_adam_state(optimizer)
        self.trainer_log['training_time'] = time.time() - start
        self.trainer_log['best_epoch'] = best_epoch
        self.trainer_log['best_valid_loss'] = best_valid_loss

    # ------------------------------------------------------------------ evaluation
    def _message_passing_edges(self, data):
        mask = data.dtrain_mask if hasattr(data, 'dtrain_mask') else data.dr_mask
        return data.train_pos_edge_index[:, mask]

    # above this many Dr edges the 500 subsets are drawn on the device (see _ensure_df_subsets)
    FAST_SUBSETS_ABOVE = 1 << 18

    def _ensure_df_subsets(self, n_dr, k, dev=None):
        """500 random Dr subsets of size |Df|, drawn once and reused (base.py:263-268 upstream).

        Up to FAST_SUBSETS_ABOVE Dr edges they are drawn exactly as upstream does - 500 x torch.randperm(n_dr) on
        the host generator, kept as boolean masks in `self.df_pos_edge` - so the same seed gives the same subsets
        (tests/test_cli_gpu.py pins them against the reference).  Beyond that (ogbl-size graphs: 2 M Dr edges make
        those 500 host permutations 19 s of a 27 s unlearning request, and the masks 1 GB) the subsets come from
        torch.randperm on the device, seeded from the host generator: the same statistic - the mean over 500
        uniformly random |Df|-subsets of Dr - from a different random stream, kept as an index matrix only."""
        if len(self.df_pos_edge) > 0:
            return
        if n_dr <= self.FAST_SUBSETS_ABOVE or dev is None or dev.type != 'cuda':
            for _ in range(500):
                chosen = torch.zeros(n_dr, dtype=torch.bool)
                chosen[torch.randperm(n_dr)[:k]] = True
                self.df_pos_edge.append(chosen)
            return
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,))))
        self._df_subset_index = torch.stack([torch.randperm(n_dr, device=dev, generator=gen)[:k] for _ in range(500)])
        self.df_pos_edge = [None] * 500          # placeholders: only the count is used on this path

    # ------------------------------------------------------------------ --fused_eval (gnndelete_amd/rankeval.py)
    def _fused_eval_applies(self, n_ref, m, k, scores):
        """Does this ranking (n_ref negatives against k-subsets of m positives, `scores` one of the score tensors) run on the
        rank kernels?  With the flag, trainer_log['eval_path'] says 'fused' or 'torch: <reason>'."""
        if not getattr(self.args, 'fused_eval', False):
            return False
        reason = fused_eval_unsupported(n_ref, m, k, scores.is_cuda, scores.dtype)
        path = 'fused' if reason is None else f'torch: {reason}'
        if reason is not None and self.trainer_log.get('eval_path') != path:
            print(f'--fused_eval: {reason}; ranking with the batched torch sort', flush=True)
        self.trainer_log['eval_path'] = path
        return reason is None

    @torch.no_grad()
    def eval(self, model, data, stage='val', pred_all=False):
        _require_gpu()
        model.eval()
        model = model.to(device)        # --eval_on_cpu existed to dodge GPU OOM; not needed with 288 GB
        data = data.to(device)
        if getattr(self.args, 'fused_validation', False):
            # --fused_validation (gnndelete_amd/evalpass.py): the request's graph and edge lists prepared once, one scoring launch
            from ... import evalpass
            out = evalpass.prepared_link_validation(self, model, data, stage, pred_all, device)
            if out is not None:
                return out                  # (None: trainer_log['validation_path'] says why, and today's path runs)
        elif getattr(self.args, 'device_subsets', False):
            from ... import evalpass
            evalpass.subset_draw(self, '--fused_validation is missing')
        pos_edge_index = data[f'{stage}_pos_edge_index']
        neg_edge_index = data[f'{stage}_neg_edge_index']
        z = model(data.x, self._message_passing_edges(data))
        logits = model.decode(z, pos_edge_index, neg_edge_index).sigmoid()
        label = self.get_link_labels(pos_edge_index, neg_edge_index)

        loss = F.binary_cross_entropy_with_logits(logits, label).cpu().item()
        n_pos = pos_edge_index.shape[1]
        fused = self._fused_eval_applies(logits.numel() - n_pos, n_pos, n_pos, logits)
        if fused:
            # --fused_eval (gnndelete_amd/rankeval.py): the stage's negatives against ALL its positives, one subset
            auc, aup = subset_auc_ap(logits[n_pos:], logits[:n_pos], torch.arange(n_pos, device=logits.device)[None])
            dt_auc, dt_aup = float(auc[0]), float(aup[0])
        else:
            # tensor AUC / AP (metrics.py): identical to scikit-learn's values, no host round trip
            dt_auc = float(batched_roc_auc(logits, label)[0])
            dt_aup = float(batched_average_precision(logits, label)[0])

        if self.args.unlearning_model in ['original']:
            df_logit = []
        elif fused:
            df_score = model.decode(z, data.directed_df_edge_index).sigmoid()        # stays on the device for the ranking
            df_logit = df_score.tolist()
        else:
            df_logit = model.decode(z, data.directed_df_edge_index).sigmoid().tolist()

        if len(df_logit) > 0 and fused:
            dr_edges = data.train_pos_edge_index[:, data.dr_mask]
            self._ensure_df_subsets(dr_edges.shape[1], len(df_logit), z.device)
            dr_score = model.decode(z, dr_edges).sigmoid()
            if getattr(self, '_df_subset_index', None) is None or self._df_subset_index.device != dr_score.device:
                self._df_subset_index = torch.stack([c.nonzero().flatten() for c in self.df_pos_edge]).to(dr_score.device)
            fused = self._fused_eval_applies(df_score.numel(), dr_score.numel(), self._df_subset_index.shape[1], dr_score)
        if len(df_logit) > 0 and fused:
            # the 500 resampled AUC / AUP from ONE sort of the Dr scores and a bitmap pass per subset: Df labelled 0, Dr labelled 1
            auc, aup = subset_auc_ap(df_score, dr_score, self._df_subset_index)
            df_auc, df_aup = float(auc.mean()), float(aup.mean())
        elif len(df_logit) > 0:
            dr_edges = data.train_pos_edge_index[:, data.dr_mask]
            self._ensure_df_subsets(dr_edges.shape[1], len(df_logit), z.device)
            # one decode over all of Dr instead of 500 decodes of subsets (same scores), then the 500
            # resampled AUC / AUP as ONE batched sort on the device: Df labelled 0, Dr labelled 1
            k = len(df_logit)
            dr_score = model.decode(z, dr_edges).sigmoid()
            if getattr(self, '_df_subset_index', None) is None or self._df_subset_index.device != dr_score.device:
                self._df_subset_index = torch.stack([c.nonzero().flatten() for c in self.df_pos_edge]).to(dr_score.device)
            df_score = torch.tensor(df_logit, dtype=dr_score.dtype, device=dr_score.device)
            scores = torch.cat([df_score[None].expand(len(self.df_pos_edge), k), dr_score[self._df_subset_index]], dim=1)
            labels = torch.cat([torch.zeros(k), torch.ones(k)]).to(dr_score.device)
            df_auc = float(batched_roc_auc(scores, labels).mean())
            df_aup = float(batched_average_precision(scores, labels).mean())
        else:
            df_auc = df_aup = np.nan

        logit_all_pair = _all_pairs(z) if pred_all else None
        log = {
            f'{stage}_loss': loss,
            f'{stage}_dt_auc': dt_auc,
            f'{stage}_dt_aup': dt_aup,
            f'{stage}_df_auc': df_auc,
            f'{stage}_df_aup': df_aup,
            f'{stage}_df_logit_mean': np.mean(df_logit) if len(df_logit) > 0 else np.nan,
            f'{stage}_df_logit_std': np.std(df_logit) if len(df_logit) > 0 else np.nan,
        }
        return loss, dt_auc, dt_aup, df_auc, df_aup, df_logit, logit_all_pair, log

    @torch.no_grad()
    def test(self, model, data, model_retrain=None, attack_model_all=None, attack_model_sub=None, ckpt='best'):
        if ckpt == 'best':
            state = torch.load(os.path.join(self.args.checkpoint_dir, 'model_best.pt'), map_location='cpu')
            model.load_state_dict(state['model_state'])
        pred_all = not is_large(self.args.dataset)       # N x N logits only for the small graphs (base.py:314-317)
        loss, dt_auc, dt_aup, df_auc, df_aup, df_logit, logit_all_pair, test_log = self.eval(model, data, 'test', pred_all)
        self.logit_all_pair = logit_all_pair
        self.trainer_log.update({
            'dt_loss': loss, 'dt_auc': dt_auc, 'dt_aup': dt_aup, 'df_logit': df_logit,
            'df_auc': df_auc, 'df_aup': df_aup, 'auc_sum': dt_auc + df_auc, 'aup_sum': dt_aup + df_aup,
            'auc_gap': abs(dt_auc - df_auc), 'aup_gap': abs(dt_aup - df_aup)})
        if model_retrain is not None:
            self.trainer_log['ve'] = verification_error(model, model_retrain).cpu().item()
        return loss, dt_auc, dt_aup, df_auc, df_aup, df_logit, logit_all_pair, test_log

    def save_log(self):
        with open(os.path.join(self.args.checkpoint_dir, 'trainer_log.json'), 'w') as f:
            json.dump(self.trainer_log, f)
        torch.save(self.logit_all_pair, os.path.join(self.args.checkpoint_dir, 'pred_proba.pt'))


class NodeClassificationTrainer(Trainer):
    """NLL node classification (base.py:694-864); eval = accuracy + micro-F1 on val_mask."""

    def _classifier_engine(self, model, data, optimizer, args):
        """The engine of one train call (--fused_backbone): Adam's hyper-parameters and state from the caller's optimizer (a
        second train call on the same model and optimizer continues the first)."""
        from ...backbone import NodeClassifierEngine
        from .gnndelete_nodeemb import _adam_hyper
        lr, betas, eps = _adam_hyper(optimizer)
        engine = NodeClassifierEngine(model, data.x, data.edge_index.contiguous(), data.y, data.train_mask, lr, betas, eps,
                                      history=max(16, args.epochs))
        engine.import_adam_state(optimizer)
        self._backbone = engine
        return engine

    def train(self, model, data, optimizer, args):
        _require_gpu()
        start = time.time()
        best_epoch, best_valid_acc = 0, 0
        model = model.to(device)
        data = data.to(device)
        engine = None
        if self._fused_backbone_applies(model, optimizer, args, task='nodecls'):
            engine = self._classifier_engine(model, data, optimizer, args)
        for epoch in range(args.epochs):
            model.train()
            if engine is not None:
                engine.step()
            else:
                z = F.log_softmax(model(data.x, data.edge_index), dim=1)
                loss = F.nll_loss(z[data.train_mask], data.y[data.train_mask])
                loss.backward()
                optimizer.step()
                optimizer.zero_grad()
            if (epoch + 1) % args.valid_freq == 0:
                if engine is not None:
                    train_loss = engine.last_loss()                 # the block's host read
                    z = F.log_softmax(engine.z, dim=1)              # this epoch's forward, as the loop keeps it
                    engine.export_adam_state(optimizer)             # (a checkpoint below carries the optimizer's state)
                else:
                    train_loss = loss.item()
                valid_loss, dt_acc, dt_f1, valid_log = self.eval(model, data, 'val')
                self._record({'epoch': epoch, 'train_loss': train_loss}, valid_log)
                if dt_acc > best_valid_acc:
                    best_valid_acc, best_epoch = dt_acc, epoch
                    print(f'Save best checkpoint at epoch {epoch:04d}. Valid Acc = {dt_acc:.4f}')
                    torch.save({'model_state': model.state_dict(), 'optimizer_state': optimizer.state_dict()},
                               os.path.join(args.checkpoint_dir, 'model_best.pt'))
                    torch.save(z.detach(), os.path.join(args.checkpoint_dir, 'node_embeddings.pt'))
        if engine is not None:
            engine.export_adam_state(optimizer)
        self.trainer_log['training_time'] = time.time() - start
        torch.save({'model_state': model.state_dict(), 'optimizer_state': optimizer.state_dict()},
                   os.path.join(args.checkpoint_dir, 'model_final.pt'))
        self.trainer_log['best_epoch'] = best_epoch
        self.trainer_log['best_valid_acc'] = best_valid_acc

    @torch.no_grad()
    def eval(self, model, data, stage='val', pred_all=False):
        _require_gpu()
        model.eval()
        model = model.to(device)
        data = data.to(device)
        if getattr(self.args, 'fused_validation', False):
            # --fused_validation (gnndelete_amd/evalpass.py): the val_mask rows listed once, loss and hit count in one launch
            from ... import evalpass
            out = evalpass.prepared_node_validation(self, model, data, stage, device)
            if out is not None:
                return out
        z = F.log_softmax(model(data.x, data.edge_index), dim=1)
        sel = data.val_mask                       # upstream reads val_mask for every stage
        loss = F.nll_loss(z[sel], data.y[sel]).cpu().item()
        pred = torch.argmax(z[sel], dim=1).cpu()
        dt_acc = accuracy_score(data.y[sel].cpu(), pred)
        dt_f1 = f1_score(data.y[sel].cpu(), pred, average='micro')
        log = {f'{stage}_loss': loss, f'{stage}_dt_acc': dt_acc, f'{stage}_dt_f1': dt_f1}
        return loss, dt_acc, dt_f1, log

    @torch.no_grad()
    def test(self, model, data, model_retrain=None, attack_model_all=None, attack_model_sub=None, ckpt='best'):
        if ckpt == 'best':
            state = torch.load(os.path.join(self.args.checkpoint_dir, 'model_best.pt'), map_location='cpu')
            model.load_state_dict(state['model_state'])
        loss, dt_acc, dt_f1, test_log = self.eval(model, data, 'test', not is_large(self.args.dataset))
        self.trainer_log.update({'dt_loss': loss, 'dt_acc': dt_acc, 'dt_f1': dt_f1})
        if model_retrain is not None:
            self.trainer_log['ve'] = verification_error(model, model_retrain).cpu().item()
        return loss, dt_acc, dt_f1, test_log
