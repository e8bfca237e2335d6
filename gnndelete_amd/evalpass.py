"""The prepared validation pass (--fused_validation; csrc/evalpass.hip; Trainer.eval and NodeClassificationTrainer.eval).

A validation of an unlearning request repeats, every --valid_freq epochs, work that depends on the request alone: the selection
train_pos_edge_index[:, mask] makes a NEW tensor each time, graph.graph_for keys its cache on tensor identity, and so every
validation rebuilds the message-passing CSR, its transpose and two SplitPlans before the four layer launches that are the
validation's own.  Here everything that depends only on the request is built once, on the first validation of a
(trainer, stage), and kept on the trainer:

  LinkValidationPlan   the message-passing edges (selected once, their graphs pinned in graph.CACHE: no LRU eviction), ONE decoded
                       edge list [stage pos | stage neg | directed Df | Dr], the [500, |Df|] subset index matrix of
                       Trainer._ensure_df_subsets (the same host-generator calls in the same order as without the flag), and a
                       staleness key over every source tensor (identity and _version): an in-place edit rebuilds the plan
  NodeValidationPlan   the int32 list of val_mask rows (upstream reads val_mask for every stage), data.edge_index pinned

and a validation is the model's own forward on the held graph (the same bits as today's z), one scoring launch pair
(gd_eval_edge_scores_f32: sigmoid scores of the whole list, the stage's loss and the Df mean / std in double; or
gd_row_nll_eval_f32: mean NLL and the arg-max hit count), rankeval.subset_auc_ap twice as under --fused_eval, and ONE host read of
the scalars (plus one tolist() of the Df scores, which stay a Python list in the returned tuple).

The scores are the kernel's own sigmoid, not torch's: the last bit of a score can differ from the no-flag path, and with it which
saturated scores tie.  Given the kernel's scores, nothing else moves: the AUCs are the doubles of metrics.batched_roc_auc on
them, the AUPs within 1e-12, loss / Df mean / Df std within 1e-12 of reference_edge_scores on them.  Values under the flag are
therefore NOT promised bit-equal to the no-flag path; a near-tie in valid_loss can select a different best epoch.

reference_edge_scores and reference_row_nll_eval restate the two entries in numpy (fp64 throughout) and are their CPU oracles.

KGTrainer.eval (R-GCN / R-GAT, DistMult) validates the same way on a KGValidationPlan: the Dr triples selected once and pinned
in graph.TYPED (ONE typed graph for conv1 and conv2 instead of one each per validation), gd_eval_triple_scores_f32 over one
decoded triple list (raw logits and BCE-with-logits for the stage, as upstream scores it; sigmoid for Df / Dr), the rank kernels
for both rankings.  Its staleness check also compares contents, because the knowledge-graph loops move the data to the host
between validations; its 500 Dr subsets stay upstream's fresh draws per call.  reference_triple_scores is that entry's oracle.

--device_subsets (gnndelete_amd/subsets.py) takes the 500 subsets out of both plans: one host randint gives a seed, and
rankeval.subset_auc_ap_drawn computes every subset's members inside the rank kernel - no permutations, no [500, |Df|] index
matrix.  The subsets come from a stream of the project's own, not from upstream's generator calls: df_auc / df_aup are the same
statistic over other subsets.  trainer_log['subset_draw'] says 'device' or 'upstream: <reason>'."""
import numpy as np
import torch

from . import rankeval, subsets

MAX_WIDTH = 256          # embedding width of gd_eval_edge_scores_f32 / classes of gd_row_nll_eval_f32


# ---------------------------------------------------------------------------------------------- numpy restatements
def _np(t, dtype=None):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t) if dtype is None else np.asarray(t, dtype=dtype)


def reference_edge_stats(scores, segments):
    """(loss, df_mean, df_std) of gd_eval_edge_scores_f32 from the scores [M] laid out by `segments` = (n_pos, n_neg, n_df, n_dr),
    fp64: loss = the mean over the stage's edges of s (1 - y) + log1p(exp(-s)) - binary_cross_entropy_with_logits applied to the
    sigmoid OUTPUTS, as upstream does; mean and population std of the Df segment (NaN when it is empty, NaN loss without stage
    edges)."""
    n_pos, n_neg, n_df, _ = (int(v) for v in segments)
    s = _np(scores).astype(np.float64).reshape(-1)
    stage, y = s[:n_pos + n_neg], np.concatenate([np.ones(n_pos), np.zeros(n_neg)])
    loss = float(np.mean(stage * (1.0 - y) + np.log1p(np.exp(-stage)))) if stage.size else float('nan')
    df = s[n_pos + n_neg:n_pos + n_neg + n_df]
    if df.size == 0:
        return loss, float('nan'), float('nan')
    mean = float(np.mean(df))
    return loss, mean, float(np.sqrt(np.mean((df - mean) ** 2)))


def reference_edge_scores(z, src, dst, segments, scores=None):
    """gd_eval_edge_scores_f32 on the CPU in numpy, fp64 throughout -> (scores64 [M], loss, df_mean, df_std).  scores64 =
    sigmoid of the fp64 dot products of the rows of z (an endpoint outside [0, n) scores logit 0).  The three statistics are
    defined on the fp32 scores the kernel stores: they are taken over `scores` when given (the kernel's output), else over
    scores64 rounded to float32."""
    z = _np(z).astype(np.float64)
    src, dst = _np(src, np.int64).reshape(-1), _np(dst, np.int64).reshape(-1)
    n = z.shape[0]
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    a, b = np.where(ok, src, 0), np.where(ok, dst, 0)
    logit = np.where(ok, np.einsum('ij,ij->i', z[a], z[b]), 0.0)
    e = np.exp(-np.abs(logit))
    s64 = np.where(logit >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    if int(sum(int(v) for v in segments)) != s64.size:
        raise ValueError(f'reference_edge_scores: segments {tuple(segments)} do not add up to {s64.size} edges')
    return (s64,) + reference_edge_stats(s64.astype(np.float32) if scores is None else scores, segments)


def reference_triple_stats(scores, segments):
    """(loss, df_mean, df_std) of gd_eval_triple_scores_f32 from the scores [M] laid out by `segments` = (n_pos, n_neg, n_df,
    n_dr), fp64.  The stage's scores are RAW logits l (KGTrainer.eval scores the stage without sigmoid): loss = the mean over
    the stage of max(l, 0) - l y + log1p(exp(-|l|)), binary_cross_entropy_with_logits (NaN without stage triples); mean and
    population std of the Df segment, which holds sigmoid outputs (NaN when it is empty)."""
    n_pos, n_neg, n_df, _ = (int(v) for v in segments)
    s = _np(scores).astype(np.float64).reshape(-1)
    stage, y = s[:n_pos + n_neg], np.concatenate([np.ones(n_pos), np.zeros(n_neg)])
    loss = float(np.mean(np.maximum(stage, 0.0) - stage * y + np.log1p(np.exp(-np.abs(stage))))) if stage.size else float('nan')
    df = s[n_pos + n_neg:n_pos + n_neg + n_df]
    if df.size == 0:
        return loss, float('nan'), float('nan')
    mean = float(np.mean(df))
    return loss, mean, float(np.sqrt(np.mean((df - mean) ** 2)))


def reference_triple_scores(z, rel, src, dst, etype, segments, scores=None):
    """gd_eval_triple_scores_f32 on the CPU in numpy, fp64 throughout -> (scores64 [M], loss, df_mean, df_std).  scores64 = the
    fp64 DistMult logits sum_j z[a, j] rel[t, j] z[b, j] for the stage's triples and their sigmoid for Df / Dr (an endpoint
    outside [0, n) or a type outside [0, n_rel) scores logit 0).  The three statistics are defined on the fp32 values the kernel
    stores: they are taken over `scores` when given (the kernel's output), else over scores64 rounded to float32."""
    z, rel = _np(z).astype(np.float64), _np(rel).astype(np.float64)
    src, dst, etype = (_np(t, np.int64).reshape(-1) for t in (src, dst, etype))
    n, n_rel = z.shape[0], rel.shape[0]
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n) & (etype >= 0) & (etype < n_rel)
    a, b, t = np.where(ok, src, 0), np.where(ok, dst, 0), np.where(ok, etype, 0)
    logit = np.where(ok, np.einsum('ij,ij,ij->i', z[a], rel[t], z[b]), 0.0)
    if int(sum(int(v) for v in segments)) != logit.size:
        raise ValueError(f'reference_triple_scores: segments {tuple(segments)} do not add up to {logit.size} triples')
    e = np.exp(-np.abs(logit))
    s64 = np.where(logit >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    n_stage = int(segments[0]) + int(segments[1])
    s64[:n_stage] = logit[:n_stage]
    return (s64,) + reference_triple_stats(s64.astype(np.float32) if scores is None else scores, segments)


def reference_row_nll_eval(z, rows, y, d_valid=None):
    """gd_row_nll_eval_f32 on the CPU in numpy, fp64 throughout -> (mean NLL, number of listed rows whose arg-max is the label).
    The arg-max takes the lowest index among equal maxima (numpy's rule); a row id outside [0, n_rows) is skipped and a label
    outside [0, d_valid) counts as wrong with term 0 (both still count in the divisor); no rows: (NaN, 0)."""
    z, rows, y = _np(z).astype(np.float64), _np(rows, np.int64).reshape(-1), _np(y, np.int64).reshape(-1)
    d_valid = z.shape[1] if d_valid is None else int(d_valid)
    if rows.size == 0:
        return float('nan'), 0
    total, correct = 0.0, 0
    for u in rows:
        if not 0 <= u < z.shape[0] or not 0 <= y[u] < d_valid:
            continue
        row = z[u, :d_valid]
        m = row.max()
        total += m + np.log(np.sum(np.exp(row - m))) - row[y[u]]
        correct += int(np.argmax(row) == y[u])
    return float(total / rows.size), int(correct)


# ---------------------------------------------------------------------------------------------- the two entries
def eval_edge_scores(z, src, dst, segments, check=True, out=None):
    """gd_eval_edge_scores_f32 on device tensors -> (scores float32 [M], stats float64 [3] = loss / Df mean / Df std, status int32
    [1]).  z: float32 [n, d], d a multiple of 4 up to 256, rows 16-byte aligned; src / dst: int64 [M] laid out by `segments` =
    (n_pos, n_neg, n_df, n_dr).  check=True reads the status (a host sync) and raises IndexError on an endpoint outside [0, n);
    with check=False the caller reads status itself (the trainer packs it into its one host read).  out: a contiguous float32 [M]
    tensor on the device of z that receives the scores (default: a new one)."""
    from . import _lib
    from ._lib import check as check_rc, ptr, stream_ptr
    n_pos, n_neg, n_df, n_dr = (int(v) for v in segments)
    if z.dim() != 2 or z.dtype != torch.float32 or not z.is_cuda or z.stride(1) != 1:
        raise ValueError('eval_edge_scores: z must be a float32 matrix with contiguous rows on the GPU')
    for name, t in (('src', src), ('dst', dst)):
        if t.dtype != torch.int64 or t.dim() != 1 or t.device != z.device or t.numel() != n_pos + n_neg + n_df + n_dr:
            raise ValueError(f'eval_edge_scores: {name} must be int64 [{n_pos + n_neg + n_df + n_dr}] on the device of z')
    src, dst = src.contiguous(), dst.contiguous()
    dev, (n, d), m_all = z.device, z.shape, src.numel()
    L = _lib.lib()
    if out is not None and (out.dtype != torch.float32 or out.device != dev or out.dim() != 1 or out.numel() != m_all or not out.is_contiguous()):
        raise ValueError(f'eval_edge_scores: out must be a contiguous float32 [{m_all}] on the device of z')
    scores = torch.empty(m_all, dtype=torch.float32, device=dev) if out is None else out
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(2, int(L.gd_eval_edge_scores_workspace(m_all, d))), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check_rc(L.gd_eval_edge_scores_f32(ptr(z), z.stride(0), n, d, ptr(src), ptr(dst), n_pos, n_neg, n_df, n_dr, ptr(scores), ptr(stats),
                                           ptr(status), ptr(ws), stream_ptr(dev)), 'gd_eval_edge_scores_f32')
    if check and int(status):
        raise IndexError(f'eval_edge_scores: an edge has an endpoint outside [0, {n})')
    return scores, stats, status


def eval_triple_scores(z, rel, src, dst, etype, segments, check=True, out=None):
    """gd_eval_triple_scores_f32 on device tensors -> (scores float32 [M], stats float64 [3] = loss / Df mean / Df std, status
    int32 [1]).  z: float32 [n, d], rel: float32 [n_rel, d] (the DistMult table), d a multiple of 4 up to 256, rows 16-byte
    aligned; src / dst / etype: int64 [M] laid out by `segments` = (n_pos, n_neg, n_df, n_dr).  The stage's scores are the raw
    logits, the Df / Dr scores their sigmoid.  check=True reads the status (a host sync) and raises IndexError on an endpoint
    outside [0, n) or a type outside [0, n_rel); out: as eval_edge_scores."""
    from . import _lib
    from ._lib import check as check_rc, ptr, stream_ptr
    n_pos, n_neg, n_df, n_dr = (int(v) for v in segments)
    if z.dim() != 2 or z.dtype != torch.float32 or not z.is_cuda or z.stride(1) != 1:
        raise ValueError('eval_triple_scores: z must be a float32 matrix with contiguous rows on the GPU')
    if rel.dim() != 2 or rel.dtype != torch.float32 or rel.device != z.device or rel.stride(1) != 1 or rel.shape[1] != z.shape[1]:
        raise ValueError(f'eval_triple_scores: rel must be a float32 [n_rel, {z.shape[1]}] matrix with contiguous rows on the device of z')
    for name, t in (('src', src), ('dst', dst), ('etype', etype)):
        if t.dtype != torch.int64 or t.dim() != 1 or t.device != z.device or t.numel() != n_pos + n_neg + n_df + n_dr:
            raise ValueError(f'eval_triple_scores: {name} must be int64 [{n_pos + n_neg + n_df + n_dr}] on the device of z')
    src, dst, etype = src.contiguous(), dst.contiguous(), etype.contiguous()
    dev, (n, d), m_all = z.device, z.shape, src.numel()
    L = _lib.lib()
    if out is not None and (out.dtype != torch.float32 or out.device != dev or out.dim() != 1 or out.numel() != m_all or not out.is_contiguous()):
        raise ValueError(f'eval_triple_scores: out must be a contiguous float32 [{m_all}] on the device of z')
    scores = torch.empty(m_all, dtype=torch.float32, device=dev) if out is None else out
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(2, int(L.gd_eval_triple_scores_workspace(m_all, d))), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check_rc(L.gd_eval_triple_scores_f32(ptr(z), z.stride(0), n, d, ptr(rel), rel.stride(0), rel.shape[0], ptr(src), ptr(dst), ptr(etype),
                                             n_pos, n_neg, n_df, n_dr, ptr(scores), ptr(stats), ptr(status), ptr(ws), stream_ptr(dev)),
                 'gd_eval_triple_scores_f32')
    if check and int(status):
        raise IndexError(f'eval_triple_scores: a triple has an endpoint outside [0, {n}) or a type outside [0, {rel.shape[0]})')
    return scores, stats, status


def row_nll_eval(z, rows, y, d_valid=None):
    """gd_row_nll_eval_f32 on device tensors -> out, a float64 [2] device tensor: out[0] the mean NLL of log_softmax(z[:, :d_valid])
    over the listed rows, out[1] the BITS of the int64 number of listed rows whose arg-max (lowest index among equal maxima) is
    the label - read_row_nll_eval(out) reads both in one host copy.  z: float32 [n_rows, >= d_valid], contiguous rows; rows: int32
    [n_sel]; y: int64 [n_rows]."""
    from . import _lib
    from ._lib import check as check_rc, ptr, stream_ptr
    d_valid = z.shape[1] if d_valid is None else int(d_valid)
    if z.dim() != 2 or z.dtype != torch.float32 or not z.is_cuda or (z.shape[1] > 1 and z.stride(1) != 1):
        raise ValueError('row_nll_eval: z must be a float32 matrix with contiguous rows on the GPU')
    if rows.dtype != torch.int32 or rows.dim() != 1 or rows.device != z.device:
        raise ValueError('row_nll_eval: rows must be an int32 vector on the device of z')
    if y.dtype != torch.int64 or y.dim() != 1 or y.device != z.device or y.numel() != z.shape[0]:
        raise ValueError('row_nll_eval: y must be int64 [n_rows] on the device of z')
    rows, y = rows.contiguous(), y.contiguous()
    dev, n_sel = z.device, rows.numel()
    L = _lib.lib()
    out = torch.empty(2, dtype=torch.float64, device=dev)
    ws = torch.empty(max(2, int(L.gd_row_nll_eval_workspace(n_sel, d_valid))), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check_rc(L.gd_row_nll_eval_f32(ptr(z), z.stride(0), z.shape[0], d_valid, ptr(rows) if n_sel else None, n_sel, ptr(y), out.data_ptr(),
                                       out.data_ptr() + 8, ptr(ws), stream_ptr(dev)), 'gd_row_nll_eval_f32')
    return out


def read_row_nll_eval(out):
    """(mean NLL as a float, hit count as an int) of row_nll_eval's device pair: one host copy."""
    host = out.cpu()
    return float(host[0]), int(host.view(torch.int64)[1])


# ---------------------------------------------------------------------------------------------- what the pass takes
def validation_unsupported(model, task='linkpred', width=None, dtype=torch.float32, on_gpu=True, rankings=()):
    """None when the prepared validation pass takes this validation, else the reason (one line).  task: 'linkpred' (Trainer.eval) or
    'nodecls' (NodeClassificationTrainer.eval); width, dtype, on_gpu: of the embeddings / logits of the model's forward (width
    None: only the model and the rankings are looked at); rankings: (n_ref, m, k) of every rankeval.subset_auc_ap call the
    validation would make."""
    if task not in ('linkpred', 'nodecls'):
        raise ValueError(f'validation_unsupported: task {task!r} (linkpred or nodecls)')
    from .framework.models.backbones import _Homogeneous
    what = 'embeddings' if task == 'linkpred' else 'logits'
    if not isinstance(model, _Homogeneous):
        return f'no prepared validation for the {type(model).__name__} model (the homogeneous two-layer backbones and their Delete wrappers only)'
    if width is not None:
        width = int(width)
        if not on_gpu:
            return f'the {what} are not on the GPU'
        if dtype != torch.float32:
            return f'{dtype} {what} (float32 only)'
        if task == 'linkpred' and (width % 4 or not 4 <= width <= MAX_WIDTH):
            return f'embedding width {width} (a multiple of 4 up to {MAX_WIDTH})'
        if task == 'nodecls' and not 1 <= width <= MAX_WIDTH:
            return f'{width} classes (the scoring kernel takes up to {MAX_WIDTH})'
    for n_ref, m, k in rankings:
        reason = rankeval.fused_eval_unsupported(n_ref, m, k)
        if reason is not None:
            return reason
    return None


def kg_validation_unsupported(model, width=None, dtype=torch.float32, on_gpu=True, rankings=()):
    """None when the prepared knowledge-graph validation takes this validation (KGTrainer.eval), else the reason (one line).
    model: RGCN / RGAT or their Delete wrappers; width, dtype, on_gpu: of the embeddings of the model's forward and of its
    DistMult table (width None: only the model and the rankings are looked at); rankings: as validation_unsupported."""
    from .framework.models.backbones import RGCN
    if not isinstance(model, RGCN):
        return f'no prepared knowledge-graph validation for the {type(model).__name__} model (RGCN, RGAT and their Delete wrappers only)'
    if width is not None:
        width = int(width)
        if not on_gpu:
            return 'the embeddings or the DistMult table are not on the GPU'
        if dtype != torch.float32:
            return f'{dtype} embeddings or DistMult table (float32 only)'
        if width % 4 or not 4 <= width <= MAX_WIDTH:
            return f'DistMult width {width} (a multiple of 4 up to {MAX_WIDTH})'
    for n_ref, m, k in rankings:
        reason = rankeval.fused_eval_unsupported(n_ref, m, k)
        if reason is not None:
            return reason
    return None


def _stamp(*tensors):
    return tuple((id(t), t._version) if torch.is_tensor(t) else None for t in tensors)


# ---------------------------------------------------------------------------------------------- link prediction
class LinkValidationPlan:
    """Everything of a link-prediction validation that depends only on the request; one per (Trainer, stage)."""

    N_SUBSETS = 500

    @staticmethod
    def sources(data, stage, original):
        """The tensors the plan is derived from, in the order of its staleness key."""
        mask = data.dtrain_mask if hasattr(data, 'dtrain_mask') else data.dr_mask
        return (data.train_pos_edge_index, mask, data[f'{stage}_pos_edge_index'], data[f'{stage}_neg_edge_index'],
                None if original else data.directed_df_edge_index, None if original else data.dr_mask)

    @classmethod
    def key_of(cls, data, stage, original, device):
        """Identity and _version of every source tensor, and the device: an in-place edit of any of them, or another tensor in
        its place, gives another key."""
        return (stage, bool(original), str(device)) + _stamp(*cls.sources(data, stage, original))

    def __init__(self, trainer, data, stage, device):
        from . import graph
        original = trainer.args.unlearning_model in ['original']
        self.stage, self.original, self.device = stage, original, device
        self.key = self.key_of(data, stage, original, device)
        self._sources = self.sources(data, stage, original)          # (kept alive: an id cannot be recycled under the key)
        train, mask, pos, neg, df, dr_mask = self._sources
        self.edges = train[:, mask].contiguous()                     # the message-passing edges, selected ONCE
        self._cache = graph.CACHE
        self._cache.pin(self.edges)                                  # their graphs are built on first use and held, outside the LRU
        self._pinned = True
        parts = [pos, neg] + ([] if original else [df, train[:, dr_mask]])
        self.segments = tuple(int(p.shape[1]) for p in parts) + ((0, 0) if original else ())
        decoded = torch.cat(parts, dim=1).long().contiguous()        # int64 [2, M]: [stage pos | stage neg | directed Df | Dr]
        self.decoded, self.src, self.dst = decoded, decoded[0], decoded[1]
        n_pos, n_neg, n_df, n_dr = self.segments
        self.all_positives = torch.arange(n_pos, device=decoded.device)[None]
        self.subset_index = self.subset_seed = None
        # --device_subsets: no index matrix and none of Trainer._ensure_df_subsets's draws; validate() draws ONE seed
        self.drawn = bool(getattr(trainer.args, 'device_subsets', False)) and n_df > 0 and subsets.device_subsets_unsupported(n_dr, n_df) is None
        if n_df > 0 and not self.drawn:
            # exactly Trainer.eval's calls: the same draws from the host generator in the same order
            trainer._ensure_df_subsets(n_dr, n_df, decoded.device)
            if getattr(trainer, '_df_subset_index', None) is None or trainer._df_subset_index.device != decoded.device:
                trainer._df_subset_index = torch.stack([c.nonzero().flatten() for c in trainer.df_pos_edge]).to(decoded.device)
            self.subset_index = trainer._df_subset_index
        self.z = self.scores = None                                  # of the latest validation

    def rankings(self):
        n_pos, n_neg, n_df, n_dr = self.segments
        return [(n_neg, n_pos, n_pos)] + ([(n_df, n_dr, n_df if self.drawn else self.subset_index.shape[1])] if n_df > 0 else [])

    def release(self):
        if getattr(self, '_pinned', False):
            self._pinned = False
            self._cache.unpin(self.edges)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    @torch.no_grad()
    def validate(self, model, data, pred_all=False, z=None):
        """One validation -> Trainer.eval's tuple.  z: model(data.x, self.edges) when the caller has already run it."""
        from .framework.trainer.base import _all_pairs
        stage = self.stage
        n_pos, n_neg, n_df, n_dr = self.segments
        n_stage = n_pos + n_neg
        if z is None:
            z = model(data.x, self.edges)
        scores, stats, status = eval_edge_scores(z, self.src, self.dst, self.segments, check=False)
        self.z, self.scores = z, scores
        auc, aup = rankeval.subset_auc_ap(scores[n_pos:n_stage], scores[:n_pos], self.all_positives)
        parts = [stats, status.double(), auc, aup]
        if n_df > 0:
            df_score = scores[n_stage:n_stage + n_df]
            if self.drawn:
                if self.subset_seed is None:
                    # the plan's ONE host call, the one the large-pool branch of Trainer._ensure_df_subsets makes; the seed is
                    # the plan's, so every validation of the request ranks the same 500 subsets, as today
                    self.subset_seed = int(torch.randint(0, 2 ** 31 - 1, (1,)))
                auc, aup = rankeval.subset_auc_ap_drawn(df_score, scores[n_stage + n_df:], self.subset_seed, 0, self.N_SUBSETS, n_df)
            else:
                auc, aup = rankeval.subset_auc_ap(df_score, scores[n_stage + n_df:], self.subset_index)
            parts += [auc.mean()[None], aup.mean()[None]]
        host = torch.cat(parts).tolist()                             # the validation's ONE read of its scalars
        if host[3] != 0.0:
            raise IndexError(f'--fused_validation: an edge of the {stage} validation has an endpoint outside [0, {z.shape[0]})')
        loss, dt_auc, dt_aup = host[0], host[4], host[5]
        df_logit = df_score.tolist() if n_df > 0 else []
        df_auc, df_aup = (host[6], host[7]) if n_df > 0 else (np.nan, np.nan)
        logit_all_pair = _all_pairs(z) if pred_all else None
        log = {
            f'{stage}_loss': loss,
            f'{stage}_dt_auc': dt_auc,
            f'{stage}_dt_aup': dt_aup,
            f'{stage}_df_auc': df_auc,
            f'{stage}_df_aup': df_aup,
            f'{stage}_df_logit_mean': host[1] if n_df > 0 else np.nan,
            f'{stage}_df_logit_std': host[2] if n_df > 0 else np.nan,
        }
        return loss, dt_auc, dt_aup, df_auc, df_aup, df_logit, logit_all_pair, log


# ---------------------------------------------------------------------------------------------- node classification
class NodeValidationPlan:
    """The val_mask rows of a node-classification validation (upstream reads val_mask for every stage); one per Trainer."""

    @staticmethod
    def key_of(data, device):
        return (str(device),) + _stamp(data.val_mask, data.y, data.edge_index)

    def __init__(self, data, device):
        from . import graph
        self.key = self.key_of(data, device)
        self._sources = (data.val_mask, data.y, data.edge_index)
        self.rows = data.val_mask.nonzero().flatten().to(torch.int32).contiguous()
        self.n_sel = int(self.rows.numel())
        self.edges = data.edge_index
        self._cache = graph.CACHE
        self._cache.pin(self.edges)
        self._pinned = True
        self.z = None

    release, __del__ = LinkValidationPlan.release, LinkValidationPlan.__del__

    @torch.no_grad()
    def validate(self, model, data, stage, z=None):
        """One validation -> NodeClassificationTrainer.eval's tuple.  dt_f1 = dt_acc: the micro-averaged F1 of a single-label
        multiclass prediction is its accuracy (every wrong row is one false positive and one false negative)."""
        if z is None:
            z = model(data.x, self.edges)
        self.z = z
        loss, correct = read_row_nll_eval(row_nll_eval(z if z.stride(1) == 1 else z.contiguous(), self.rows, data.y))
        dt_acc = correct / self.n_sel if self.n_sel else float('nan')
        dt_f1 = dt_acc
        log = {f'{stage}_loss': loss, f'{stage}_dt_acc': dt_acc, f'{stage}_dt_f1': dt_f1}
        return loss, dt_acc, dt_f1, log


# ---------------------------------------------------------------------------------------------- knowledge graphs
class KGValidationPlan:
    """Everything of a knowledge-graph validation (KGTrainer.eval) that depends only on the request; one per (trainer, stage):
    the Dr message-passing edges and types, selected ONCE and pinned in graph.TYPED (one typed graph for conv1 and conv2, held
    while the batches' graphs pass through the convs), the decoded triple list [stage pos | stage neg | directed Df | Dr] with
    its segments, and the stage's all-positives row.

    The knowledge-graph loops move the data to the host between validations (data.to('cpu'), then eval's data.to(device)), so
    every validation presents NEW tensors: the staleness check (current) first compares identity and _version of every source
    as LinkValidationPlan does, and where that differs but shapes, dtypes and device agree it compares the CONTENTS exactly
    against the sources the plan holds (elementwise equality reduced to one flag, one host read; no hash).  Equal contents adopt
    the new tensors as the plan's sources and keep everything derived; anything else rebuilds.

    The 500 Dr subsets are NOT the plan's: upstream draws them fresh on every call, and validate() makes the same generator
    calls in the same order as KGTrainer.eval, so a seed gives the same subsets and leaves the same host random stream.  Under
    --device_subsets (validate(drawn=True)) a validation makes ONE of those calls, the large-pool branch's randint, and the
    rank kernel draws the subsets from its value (subsets.py): subset_seed holds it, subsets stays None."""

    N_SUBSETS = 500

    @staticmethod
    def sources(data, stage, original):
        """The tensors the plan is derived from, in the order of its staleness key."""
        dfdr = () if original else (data.directed_df_edge_index, data.directed_df_edge_type, data.train_pos_edge_index, data.train_edge_type)
        return (data.edge_index, data.edge_type, data.dr_mask, data[f'{stage}_pos_edge_index'], data[f'{stage}_neg_edge_index'],
                data[f'{stage}_edge_type']) + dfdr

    @classmethod
    def key_of(cls, data, stage, original, device):
        return (stage, bool(original), str(device)) + _stamp(*cls.sources(data, stage, original))

    def __init__(self, trainer, data, stage, device):
        from . import graph
        original = trainer.args.unlearning_model in ['original']
        self.stage, self.original, self.device = stage, original, device
        self.key = self.key_of(data, stage, original, device)
        self._sources = self.sources(data, stage, original)          # held: what a later validation's tensors are compared with
        edge_index, edge_type, dr_mask, pos, neg, etype = self._sources[:6]
        self.edges = edge_index[:, dr_mask].contiguous()             # the message-passing triples, selected ONCE
        self.types = edge_type[dr_mask].contiguous()
        self._registry = graph.TYPED
        self._registry.pin(self.edges, self.types)                   # their typed graph is built on first use and held, shared by the convs
        self._pinned = True
        parts, types = [pos, neg], [etype, etype]
        if not original and data.directed_df_edge_index.shape[1] > 0:
            df, df_type, train, train_type = self._sources[6:]
            half = dr_mask[:dr_mask.shape[0] // 2]
            parts += [df, train[:, half]]
            types += [df_type, train_type[half]]
        self.segments = tuple(int(p.shape[1]) for p in parts) + ((0, 0) if len(parts) == 2 else ())
        decoded = torch.cat(parts, dim=1).long().contiguous()        # int64 [2, M]: [stage pos | stage neg | directed Df | Dr]
        self.decoded, self.src, self.dst = decoded, decoded[0], decoded[1]
        self.etype = torch.cat(types, dim=0).long().contiguous()
        self.all_positives = torch.arange(self.segments[0], device=decoded.device)[None]
        self.z = self.scores = self.subsets = self.subset_seed = None   # of the latest validation

    def current(self, data, stage, original, device):
        """Is the plan still that of (data, stage)?  True on an identity hit, or after adopting tensors of equal contents."""
        key = self.key_of(data, stage, original, device)
        if key == self.key:
            return True
        if key[:3] != self.key[:3]:
            return False
        new, equal = self.sources(data, stage, original), []
        for old, stamp, t in zip(self._sources, self.key[3:], new):
            if old is t and stamp == (id(t), t._version):
                continue
            # an in-place edit (of the tensor presented, or of the one held) is not compared: the held values are no longer
            # the ones the plan was derived from
            if old is t or old._version != stamp[1] or t.shape != old.shape or t.dtype != old.dtype or t.device != old.device:
                return False
            equal.append((t == old).all())
        if not bool(torch.stack(equal).all()):                       # ONE host read
            return False
        self._sources, self.key = new, key
        return True

    def rankings(self):
        n_pos, n_neg, n_df, n_dr = self.segments
        return [(n_neg, n_pos, n_pos)] + ([(n_df, n_dr, n_df)] if n_df > 0 else [])

    def release(self):
        if getattr(self, '_pinned', False):
            self._pinned = False
            self._registry.unpin(self.edges, self.types)

    __del__ = LinkValidationPlan.__del__

    def _draw_subsets(self, trainer, n_dr, k, dev):
        """KGTrainer.eval's draws, call for call: 500 host permutations up to FAST_SUBSETS_ABOVE pool scores, beyond it one host
        randint seeding 500 device permutations."""
        if n_dr <= trainer.FAST_SUBSETS_ABOVE:
            return torch.stack([torch.randperm(n_dr)[:k].sort().values for _ in range(self.N_SUBSETS)]).to(dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,))))
        picks = torch.empty(self.N_SUBSETS, k, dtype=torch.int64, device=dev)
        for row in picks:                # the same draws, copied row by row: a list of [:k] views would hold all 500 permutations
            row.copy_(torch.randperm(n_dr, device=dev, generator=gen)[:k])
        return picks

    @torch.no_grad()
    def validate(self, trainer, model, data, pred_all=False, z=None, drawn=False):
        """One validation -> KGTrainer.eval's tuple.  z: model(data.x, self.edges, self.types) when the caller has run it;
        drawn: --device_subsets applies (the 500 subsets come from subsets.py's stream inside the rank kernel)."""
        from .framework.trainer.base import _all_pairs
        stage = self.stage
        n_pos, n_neg, n_df, n_dr = self.segments
        n_stage = n_pos + n_neg
        if z is None:
            z = model(data.x, self.edges, self.types)
        scores, stats, status = eval_triple_scores(z, model.W.detach(), self.src, self.dst, self.etype, self.segments, check=False)
        self.z, self.scores = z, scores
        auc, aup = rankeval.subset_auc_ap(scores[n_pos:n_stage], scores[:n_pos], self.all_positives)      # raw logits, as upstream
        parts = [stats, status.double(), auc, aup]
        if n_df > 0:
            df_score = scores[n_stage:n_stage + n_df]
            if drawn:
                # ONE host call, the one the large-pool branch of _draw_subsets makes: above FAST_SUBSETS_ABOVE the host random
                # stream after a validation is the one without the flag
                self.subsets, self.subset_seed = None, int(torch.randint(0, 2 ** 31 - 1, (1,)))
                auc, aup = rankeval.subset_auc_ap_drawn(df_score, scores[n_stage + n_df:], self.subset_seed, 0, self.N_SUBSETS, n_df)
            else:
                self.subsets = self._draw_subsets(trainer, n_dr, n_df, scores.device)
                auc, aup = rankeval.subset_auc_ap(df_score, scores[n_stage + n_df:], self.subsets)
            parts += [auc.mean()[None], aup.mean()[None]]
        host = torch.cat(parts).tolist()                             # the validation's ONE read of its scalars
        if host[3] != 0.0:
            raise IndexError(f'--fused_validation: a triple of the {stage} validation has an endpoint outside [0, {z.shape[0]}) or a type '
                             f'outside [0, {model.W.shape[0]})')
        loss, dt_auc, dt_aup = host[0], host[4], host[5]
        df_logit = df_score.tolist() if n_df > 0 else []
        df_auc, df_aup = (host[6], host[7]) if n_df > 0 else (np.nan, np.nan)
        logit_all_pair = _all_pairs(z) if pred_all else None
        log = {f'{stage}_loss': loss, f'{stage}_dt_auc': dt_auc, f'{stage}_dt_aup': dt_aup, f'{stage}_df_auc': df_auc,
               f'{stage}_df_aup': df_aup,
               f'{stage}_df_logit_mean': host[1] if n_df > 0 else np.nan,
               f'{stage}_df_logit_std': host[2] if n_df > 0 else np.nan}
        return loss, dt_auc, dt_aup, df_auc, df_aup, df_logit, logit_all_pair, log


# ---------------------------------------------------------------------------------------------- the trainers' entry
def subset_draw(trainer, reason):
    """Under --device_subsets: trainer_log['subset_draw'] = 'device' (reason None) or 'upstream: <reason>', a reason printed once;
    returns whether the device draws.  Without the flag: False, nothing recorded."""
    if not getattr(trainer.args, 'device_subsets', False):
        return False
    how = 'device' if reason is None else f'upstream: {reason}'
    if reason is not None and trainer.trainer_log.get('subset_draw') != how:
        print(f'--device_subsets: {reason}; drawing the validation subsets as upstream does', flush=True)
    trainer.trainer_log['subset_draw'] = how
    return reason is None


def _fallback(trainer, reason):
    path = f'torch: {reason}'
    if trainer.trainer_log.get('validation_path') != path:
        print(f'--fused_validation: {reason}; validating on the torch path', flush=True)
    trainer.trainer_log['validation_path'] = path
    subset_draw(trainer, f'the prepared pass fell back ({reason})')
    return None


def _plan(trainer, slot, key, build):
    plans = trainer.__dict__.setdefault('_validation_plans', {})
    plan = plans.get(slot)
    if plan is None or plan.key != key:
        if plan is not None:
            plan.release()
        plan = plans[slot] = build()
    return plan


def prepared_link_validation(trainer, model, data, stage, pred_all, device):
    """Trainer.eval under --fused_validation: its tuple, or None after recording why the torch path runs instead (model and
    data are on `device`, the model in eval mode).  The model is looked at before anything is built; the width and dtype of z
    are those of the forward itself, so a model whose embeddings the kernel does not take pays one forward before it falls back."""
    reason = validation_unsupported(model, 'linkpred')
    if reason is not None:
        return _fallback(trainer, reason)
    original = trainer.args.unlearning_model in ['original']
    key = LinkValidationPlan.key_of(data, stage, original, device)
    plan = _plan(trainer, ('link', stage), key, lambda: LinkValidationPlan(trainer, data, stage, device))
    z = model(data.x, plan.edges)
    reason = validation_unsupported(model, 'linkpred', z.shape[1], z.dtype, z.is_cuda, plan.rankings())
    if reason is not None:
        return _fallback(trainer, reason)
    if plan.segments[2] > 0:
        subset_draw(trainer, None if plan.drawn else subsets.device_subsets_unsupported(plan.segments[3], plan.segments[2]))
    out = plan.validate(model, data, pred_all, z)
    trainer.trainer_log['validation_path'] = 'prepared'
    return out


def prepared_kg_validation(trainer, model, data, stage, pred_all, device):
    """KGTrainer.eval under --fused_validation: its tuple, or None after recording why the torch path runs instead (model and
    data are on `device`, the model in eval mode).  The model and the width of its DistMult table are looked at before anything
    is built, and nothing is drawn from a generator before the last check: a fallback leaves the random stream to the torch
    path, which then gives exactly its no-flag values."""
    reason = kg_validation_unsupported(model)
    if reason is None:
        reason = kg_validation_unsupported(model, model.W.shape[1], model.W.dtype, model.W.is_cuda)
    if reason is not None:
        return _fallback(trainer, reason)
    original = trainer.args.unlearning_model in ['original']
    plans = trainer.__dict__.setdefault('_validation_plans', {})
    plan = plans.get(('kg', stage))
    if plan is None or not plan.current(data, stage, original, device):
        if plan is not None:
            plan.release()
        plan = plans[('kg', stage)] = KGValidationPlan(trainer, data, stage, device)
    z = model(data.x, plan.edges, plan.types)
    reason = kg_validation_unsupported(model, z.shape[1], z.dtype, z.is_cuda, plan.rankings())
    if reason is None and z.shape[1] != model.W.shape[1]:
        reason = f'embedding width {z.shape[1]} against a DistMult table of width {model.W.shape[1]}'
    if reason is not None:
        return _fallback(trainer, reason)
    n_df, n_dr = plan.segments[2:]
    drawn = n_df > 0 and subset_draw(trainer, subsets.device_subsets_unsupported(n_dr, n_df))
    out = plan.validate(trainer, model, data, pred_all, z, drawn)
    trainer.trainer_log['validation_path'] = 'prepared'
    return out


def prepared_node_validation(trainer, model, data, stage, device):
    """NodeClassificationTrainer.eval under --fused_validation: its tuple, or None after recording why the torch path runs."""
    reason = validation_unsupported(model, 'nodecls')
    if reason is not None:
        return _fallback(trainer, reason)
    plan = _plan(trainer, ('node',), NodeValidationPlan.key_of(data, device), lambda: NodeValidationPlan(data, device))
    z = model(data.x, plan.edges)
    reason = validation_unsupported(model, 'nodecls', z.shape[1], z.dtype, z.is_cuda)
    if reason is not None:
        return _fallback(trainer, reason)
    out = plan.validate(model, data, stage, z)
    trainer.trainer_log['validation_path'] = 'prepared'
    return out
