"""Shared inputs of the R-GAT attention tests (test_rgat_cases_cpu.py, test_rgat_kernels_gpu.py): softmax segments with
empty / one-entry / wave-boundary / hub rows under five logit regimes, a knowledge graph with a 1,500-edge hub target and
a 1,000-edge hub source, layer shapes for every branch of RGATConv.forward, a graph past one sweep of gd_rgcn_conv_f32's
grid and a two-layer RGATDelete state.  Everything is deterministic from seeds and fp32-representable: drawn in fp32 and
only then widened, so the fp64 reference and the kernels read the same numbers.  The references are computed once per
process (lru_cache) and must be left unchanged by their users."""
import functools

import torch
import torch.nn.functional as F

from oracle import pyg_semantics as pyg

TOL = 1e-5                      # forward values, rel-L2 to fp64 (the suite's kernel tolerance)
GRAD_TOL = 2e-5                 # gradients (test_typed_conv_with_trainable_relation_weights_matches_fp64_autograd)
SOFTMAX_FLOOR = 2.0 ** -22      # two ulps of 1.0: the floor of the per-element softmax bound
SOFTMAX_FACTOR = 8.0            # x the fp32 restatement's own error: another summation order + the fast exponential

# ---------------------------------------------------------------------------------------------------------------------
# 1. softmax segments
# ---------------------------------------------------------------------------------------------------------------------
ROW_LENGTHS = [0, 1, 63, 64, 65, 0, 128, 129, 1000, 5000, 2, 0]
PREFIXES = (1, 4, 5, len(ROW_LENGTHS))                      # a block holds four rows
REGIMES = ('randn', 'wide', 'offset', 'equal', 'dominant')


def softmax_rowptr(n_rows=len(ROW_LENGTHS)):
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor(ROW_LENGTHS[:n_rows]), 0)
    return rowptr.to(torch.int32)


@functools.lru_cache(maxsize=None)
def softmax_logits(regime):
    """fp32 logits for the whole CSR; a prefix of the rows reads a prefix of them."""
    nnz = sum(ROW_LENGTHS)
    g = torch.Generator().manual_seed(4100 + REGIMES.index(regime))
    r = torch.randn(nnz, generator=g)
    if regime == 'randn':
        return r
    if regime == 'wide':                                    # exp of the raw value overflows, most terms underflow
        return r * 40
    if regime == 'offset':
        return 3e4 + r
    if regime == 'equal':
        return torch.full((nnz,), 7.25)
    assert regime == 'dominant'
    r[::97] += 60
    return r


@functools.lru_cache(maxsize=None)
def softmax_upstream():
    return torch.randn(sum(ROW_LENGTHS), generator=torch.Generator().manual_seed(4200))


def row_of_entry(rowptr):
    lens = (rowptr[1:] - rowptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(lens.numel()), lens)


def softmax_reference(regime, n_rows, dtype):
    """(alpha, de) of pyg.segment_softmax and its autograd in `dtype` on the first n_rows rows."""
    rowptr = softmax_rowptr(n_rows)
    nnz = int(rowptr[-1])
    e = softmax_logits(regime)[:nnz].to(dtype).clone().requires_grad_()
    alpha = pyg.segment_softmax(e, row_of_entry(rowptr), n_rows)
    if nnz:
        alpha.backward(softmax_upstream()[:nnz].to(dtype))
    return alpha.detach(), (e.grad if nnz else torch.zeros_like(e))


def softmax_errors(alpha, de, regime, n_rows):
    """Largest per-element absolute error of alpha (alphas are at most 1) and of de scaled by its row's max |dalpha|,
    against the fp64 reference, and the largest |row sum - 1| over the non-empty rows."""
    rowptr = softmax_rowptr(n_rows)
    nnz = int(rowptr[-1])
    if nnz == 0:
        return 0.0, 0.0, 0.0
    a64, d64 = softmax_reference_fp64(regime, n_rows)
    rows = row_of_entry(rowptr)
    up = softmax_upstream()[:nnz].double().abs()
    scale = torch.zeros(n_rows, dtype=torch.float64).scatter_reduce(0, rows, up, reduce='amax', include_self=True)[rows]
    sums = torch.zeros(n_rows, dtype=torch.float64).index_add(0, rows, alpha.double())
    nonempty = (rowptr[1:] - rowptr[:-1]) > 0
    return (float((alpha.double() - a64).abs().max()), float(((de.double() - d64).abs() / scale).max()),
            float((sums[nonempty] - 1).abs().max()))


@functools.lru_cache(maxsize=None)
def softmax_reference_fp64(regime, n_rows):
    return softmax_reference(regime, n_rows, torch.float64)


@functools.lru_cache(maxsize=None)
def softmax_restatement_errors(regime, n_rows):
    """The errors of the SAME formula restated in fp32 on the host: what the kernel's bound is measured from."""
    a32, d32 = softmax_reference(regime, n_rows, torch.float32)
    return softmax_errors(a32, d32, regime, n_rows)


def softmax_rowwise_fp32(regime, n_rows):
    """The same formula in fp32 with every row summed by torch.sum (pairwise) instead of index_add's one-by-one order: the
    summation order that the row-sum check can be met with in fp32 (index_add's drifts by 2e-6 over 5,000 entries)."""
    rowptr = softmax_rowptr(n_rows).tolist()
    e = softmax_logits(regime)
    alpha = torch.zeros(rowptr[-1])
    for s, t in zip(rowptr[:-1], rowptr[1:]):
        if t > s:
            ex = torch.exp(e[s:t] - e[s:t].max())
            alpha[s:t] = ex / (ex.sum() + 1e-16)
    return alpha


def softmax_bounds(regime, n_rows):
    ea, ed, _ = softmax_restatement_errors(regime, n_rows)
    return max(SOFTMAX_FACTOR * ea, SOFTMAX_FLOOR), max(SOFTMAX_FACTOR * ed, SOFTMAX_FLOOR)


# ---------------------------------------------------------------------------------------------------------------------
# 2. knowledge graph with hubs
# ---------------------------------------------------------------------------------------------------------------------
N_NODES, N_REL, N_ISOLATED = 2000, 7, 50
HUB_IN, HUB_OUT = 17, 23
SELF_LOOPS = (5, HUB_IN, HUB_OUT, 100, 1949)


@functools.lru_cache(maxsize=None)
def hub_graph():
    """-> (edge_index [2, E], edge_type [E]): 1,500 in-edges onto node 17, 1,000 out-edges from node 23, 3,000 random
    edges, the first 100 of them twice (multi-edges, same relation), five self loops; no in-edge onto the last 50 nodes;
    types uniform over the first six of seven relations."""
    g = torch.Generator().manual_seed(1723)
    lim = N_NODES - N_ISOLATED
    hub_in = torch.stack([torch.randint(0, N_NODES, (1500,), generator=g), torch.full((1500,), HUB_IN)])
    hub_out = torch.stack([torch.full((1000,), HUB_OUT), torch.randint(0, lim, (1000,), generator=g)])
    rnd = torch.randint(0, lim, (2, 3000), generator=g)
    loops = torch.tensor(SELF_LOOPS).expand(2, -1)
    et = torch.randint(0, N_REL - 1, (1500 + 1000 + 3000 + len(SELF_LOOPS),), generator=g)
    ei = torch.cat([hub_in, hub_out, rnd, loops, rnd[:, :100]], 1)
    et = torch.cat([et, et[2500:2600]])
    return ei.contiguous(), et.contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# 3. / 4. layer shapes
# ---------------------------------------------------------------------------------------------------------------------
KERNEL_SHAPES = [(128, 64, 4), (64, 128, 4), (16, 8, None)]
FALLBACK_SHAPES = [(12, 12, 4), (132, 8, None)]             # block width 3 (odd); input above 128
WIDE_SHAPE = (128, 64, 4)
WIDE_MIN_SPAN = 176.0                                       # twice the range of fp32 exp
GRAD_NAMES = ('x', 'weight', 'q', 'k', 'bias')


@functools.lru_cache(maxsize=None)
def layer_case(d_in, d_out, nb, wide=False):
    """fp32 inputs of one RGATConv on the hub graph; `wide` multiplies q and k by 4 (exact in fp32)."""
    g = torch.Generator().manual_seed(7 * d_in + d_out)
    x = torch.randn(N_NODES, d_in, generator=g)
    if nb is None:
        weight = torch.randn(N_REL, d_in, d_out, generator=g) * 0.2
    else:
        weight = torch.randn(N_REL, nb, d_in // nb, d_out // nb, generator=g) * 0.2
    q, k = torch.randn(d_out, 1, generator=g), torch.randn(d_out, 1, generator=g)
    bias = torch.randn(d_out, generator=g) + 0.25
    gy = torch.randn(N_NODES, d_out, generator=g)
    if wide:
        q, k = q * 4, k * 4
    return dict(x=x, weight=weight, q=q, k=k, bias=bias, gy=gy)


def rgat_logits(x, edge_index, edge_type, weight, q, k, nb, slope=0.2):
    """The attention logits of rgat_conv, e = leaky_relu(x_i W_r q + x_j W_r k), through the two [N, R] tables."""
    r = weight.shape[0]
    if nb is None:
        wq, wk = (weight @ q).squeeze(-1), (weight @ k).squeeze(-1)
    else:
        wq = torch.einsum('rbio,bo->rbi', weight, q.view(nb, -1)).reshape(r, -1)
        wk = torch.einsum('rbio,bo->rbi', weight, k.view(nb, -1)).reshape(r, -1)
    a, b = x @ wq.t(), x @ wk.t()
    return F.leaky_relu(a[edge_index[1], edge_type] + b[edge_index[0], edge_type], slope)


def _layer_reference(d_in, d_out, nb, wide, dtype):
    c = layer_case(d_in, d_out, nb, wide)
    ei, et = hub_graph()
    leaves = {n: c[n].to(dtype).clone().requires_grad_() for n in GRAD_NAMES}
    y = pyg.rgat_conv(leaves['x'], ei, et, leaves['weight'], leaves['q'], leaves['k'], leaves['bias'], nb)
    y.backward(c['gy'].to(dtype))
    out = {'y': y.detach()}
    out.update({'d' + n: leaves[n].grad for n in GRAD_NAMES})
    return out


@functools.lru_cache(maxsize=None)
def layer_reference_fp64(d_in, d_out, nb, wide=False):
    """y and the gradients of sum(y * gy) of the fp64 oracle; 'span' = max - min of its logits."""
    out = _layer_reference(d_in, d_out, nb, wide, torch.float64)
    c = layer_case(d_in, d_out, nb, wide)
    ei, et = hub_graph()
    e = rgat_logits(c['x'].double(), ei, et, c['weight'].double(), c['q'].double(), c['k'].double(), nb)
    out['span'] = float(e.max() - e.min())
    return out


@functools.lru_cache(maxsize=None)
def layer_fp32_distances(d_in, d_out, nb, wide=False):
    """rel-L2 distance of the fp32 oracle to the fp64 oracle on y and every gradient."""
    from helpers import rel_l2
    r64, r32 = layer_reference_fp64(d_in, d_out, nb, wide), _layer_reference(d_in, d_out, nb, wide, torch.float32)
    return {n: rel_l2(r32[n], r64[n]) for n in r32}


# ---------------------------------------------------------------------------------------------------------------------
# C. a graph past one sweep of gd_rgcn_conv_f32's grid (16,384 blocks x 4 rows)
# ---------------------------------------------------------------------------------------------------------------------
SWEEP = 65536
LARGE_N, LARGE_REL = SWEEP + 9, 5
LARGE_SHAPES = [(8, 8, None), (128, 64, 4)]


@functools.lru_cache(maxsize=None)
def large_graph():
    """~4,000 edges on 65,545 nodes: endpoints in rows 0-10, in rows 65,530-65,544 (both sides of the sweep boundary: rows
    65,536 ... are the second trip of the waves that own rows 0 ...) and at random; the last relation has no edge."""
    g = torch.Generator().manual_seed(6553)
    lo = lambda m: torch.randint(0, 11, (m,), generator=g)
    hi = lambda m: torch.randint(LARGE_N - 15, LARGE_N, (m,), generator=g)
    rnd = lambda m: torch.randint(0, LARGE_N, (m,), generator=g)
    parts = [(lo(300), lo(300)), (lo(300), hi(300)), (hi(300), lo(300)), (hi(300), hi(300)), (rnd(300), lo(300)), (rnd(300), hi(300)),
             (lo(300), rnd(300)), (hi(300), rnd(300)), (rnd(1600), rnd(1600))]
    ei = torch.stack([torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])])
    et = torch.randint(0, LARGE_REL - 1, (ei.shape[1],), generator=g)
    return ei.contiguous(), et.contiguous()


@functools.lru_cache(maxsize=None)
def large_case(d_in, d_out, nb):
    g = torch.Generator().manual_seed(31 * d_in + d_out)
    ei, _ = large_graph()
    blocks = nb or 1
    return dict(x=torch.randn(LARGE_N, d_in, generator=g),
                weight=torch.randn(LARGE_REL, blocks, d_in // blocks, d_out // blocks, generator=g) * 0.2,
                coef=torch.rand(ei.shape[1], generator=g) + 0.1, gy=torch.randn(LARGE_N, d_out, generator=g))


def _large_reference(d_in, d_out, nb, dtype):
    """y_i = sum over the in-edges e = (j -> i, r) of c_e x_j W_r, the plain per-edge formula, and its autograd."""
    c = large_case(d_in, d_out, nb)
    ei, et = large_graph()
    m, blocks = ei.shape[1], nb or 1
    x, w, cf = (c[n].to(dtype).clone().requires_grad_() for n in ('x', 'weight', 'coef'))
    msg = torch.einsum('ebi,ebio->ebo', x[ei[0]].view(m, blocks, -1), w[et]).reshape(m, d_out) * cf[:, None]
    y = torch.zeros(LARGE_N, d_out, dtype=dtype).index_add(0, ei[1], msg)
    y.backward(c['gy'].to(dtype))
    return dict(y=y.detach(), dx=x.grad, dweight=w.grad, dcoef=cf.grad)


@functools.lru_cache(maxsize=None)
def large_reference_fp64(d_in, d_out, nb):
    return _large_reference(d_in, d_out, nb, torch.float64)


def large_fp32_distances(d_in, d_out, nb):
    from helpers import rel_l2
    r64, r32 = large_reference_fp64(d_in, d_out, nb), _large_reference(d_in, d_out, nb, torch.float32)
    return {n: rel_l2(r32[n], r64[n]) for n in r32}


# ---------------------------------------------------------------------------------------------------------------------
# E. two-layer RGATDelete
# ---------------------------------------------------------------------------------------------------------------------
MODEL_DIMS = (64, 128, 64)              # node embedding, hidden, out
MODEL_EDGE_TYPES = 21                   # > 20: 42 relations with four diagonal blocks, the knowledge-graph configuration
MODEL_PARAMS = ['deletion1.deletion_weight', 'deletion2.deletion_weight'] + [
    f'conv{l}.{p}' for l in (1, 2) for p in ('weight', 'q', 'k', 'bias')] + ['node_emb.weight']


@functools.lru_cache(maxsize=None)
def model_case():
    """-> (state dict, mask1, mask2, u1, u2): one seeded state for the oracle and the HIP model - relation weights
    randn * 0.2, q / k randn, nonzero biases, Del weights that are no multiple of the all-ones matrix - masks that cover
    the two hubs and some rows without in-edges, and the upstream gradients of z1 and z2."""
    from oracle import gnndelete_ref as R
    g = torch.Generator().manual_seed(2117)
    i, h, o = MODEL_DIMS
    state = {k: v.clone() for k, v in R.TwoLayerDelete('rgat', i, h, o, None, None, num_nodes=N_NODES,
                                                       num_edge_type=MODEL_EDGE_TYPES).state_dict().items()}
    for name in sorted(state):
        t = state[name]
        if name.endswith(('.weight', '.q', '.k', '.bias', 'deletion_weight')) or name == 'W':
            scale = 0.2 if name.endswith('conv1.weight') or name.endswith('conv2.weight') else 1.0
            t.copy_(torch.randn(t.shape, generator=g) * scale)
        if name.endswith('deletion_weight'):
            t.mul_(0.1).add_(torch.eye(t.shape[0]))
        if name.endswith('.bias'):
            t.add_(0.25)
    mask1, mask2 = torch.rand(N_NODES, generator=g) < 0.3, torch.rand(N_NODES, generator=g) < 0.5
    for m in (mask1, mask2):
        m[[HUB_IN, HUB_OUT]] = True
        m[N_NODES - 10:N_NODES - 4] = True
    mask1[N_NODES - 4:] = False
    u1, u2 = torch.randn(N_NODES, h, generator=g), torch.randn(N_NODES, o, generator=g)
    return state, mask1, mask2, u1, u2


def _model_reference(dtype):
    """The oracle on the hub graph in `dtype`: the Del forward (conv1 frozen, as the Del trainers run it) with its
    gradients, and the plain backbone (as the backbone trainer runs it) with the gradients down to the node embedding."""
    from helpers import oracle_model
    state, mask1, mask2, u1, u2 = model_case()
    ei, et = hub_graph()
    x = torch.arange(N_NODES)
    out = {}
    for tag in ('del', 'backbone'):
        m = oracle_model('rgat', state, mask1, mask2, num_nodes=N_NODES, num_edge_type=MODEL_EDGE_TYPES).to(dtype)
        if tag == 'del':
            z1, z2 = m(x, ei, et, return_all_emb=True)
        else:
            z1, z2 = m.get_original_embeddings(x, ei, et, return_all_emb=True)
        ((z1 * u1.to(dtype)).sum() + (z2 * u2.to(dtype)).sum()).backward()
        out[tag] = dict(z1=z1.detach(), z2=z2.detach(), grads={n: p.grad for n, p in m.named_parameters() if n in MODEL_PARAMS})
    return out


@functools.lru_cache(maxsize=None)
def model_reference_fp64():
    return _model_reference(torch.float64)


def model_fp32_distances():
    from helpers import rel_l2
    r64, r32 = model_reference_fp64(), _model_reference(torch.float32)
    out = {}
    for tag in r64:
        out[f'{tag}.z1'], out[f'{tag}.z2'] = rel_l2(r32[tag]['z1'], r64[tag]['z1']), rel_l2(r32[tag]['z2'], r64[tag]['z2'])
        for n, gr in r64[tag]['grads'].items():
            if gr is not None:
                out[f'{tag}.{n}'] = rel_l2(r32[tag]['grads'][n], gr)
    return out
