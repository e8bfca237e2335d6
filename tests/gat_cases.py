"""Shared inputs of the plain-GAT attention tests (test_gat_cases_cpu.py, test_gat_kernels_gpu.py): a 6,000-node graph with
in-degrees 1 ... 5,000 and out-degrees 256 ... 1,000 at fixed node ids, two graphs whose work items outnumber one trip of the
persistent kernels' grid, six logit regimes on a 2^-10 grid, fp64 references of everything the kernels return and the SAME
formula restated in fp32 on the host, with per-row error measures that are scaled by the sum of the magnitudes a row adds up.
Everything is deterministic from seeds and fp32-representable: drawn in fp32 and only then widened, so the fp64 reference and
the kernels read the same numbers.  The references are computed once per process (lru_cache) and must be left unchanged by
their users."""
import functools
import types

import torch
import torch.nn.functional as F

from oracle import pyg_semantics as pyg
from rgat_cases import SOFTMAX_FACTOR, SOFTMAX_FLOOR      # 8 x the restatement's own error, floor 2^-22 (see rgat_cases.py)

SLOPE = float(torch.tensor(0.2, dtype=torch.float32))    # the slope the kernels receive (a float), exactly, for every dtype
GRID = 1024.0                                            # logits are multiples of 2^-10: a_src[j] + a_dst[i] is exact in fp32
SCALE_FLOOR = 1e-30                                      # x the largest scale of a quantity: fp32 holds no weight below 1e-38
ROWMAX_ULPS = 2.0
REGIMES = ('randn', 'wide', 'negative', 'zero', 'dominant_tail', 'dominant_head')
WIDTHS = (4, 8, 16, 32, 64, 128, 256, 512, 1024)         # every instance of the balanced kernels
REGIME_WIDTHS = (8, 64, 128, 512)                        # every regime runs at these
ROW_KERNEL_WIDTHS = (20, 64, 260)
SUBSET_WIDTHS = VISIT_WIDTHS = (64, 16)


def balanced_cases():
    """(d, regime) of sections A and B: every width under randn and dominant_tail, every regime at four widths."""
    out = [(d, r) for d in WIDTHS for r in ('randn', 'dominant_tail')]
    return out + [(d, r) for d in REGIME_WIDTHS for r in REGIMES if (d, r) not in out]


# ---------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------
# degrees as build_csr(..., 'gat') sees them: with the loop it appends
HUB_IN = {100: 1, 200: 2, 300: 63, 400: 64, 500: 65, 600: 128, 700: 129, 800: 256, 900: 257, 1000: 320, 1100: 1000, 1200: 5000}
HUB_OUT = {1300: 256, 1400: 257, 1500: 300, 1600: 1000}
SPEC = {
    'hub': dict(n=6000, isolated=50, hub_in=HUB_IN, hub_out=HUB_OUT, background=4000, seed=6001),
    # hubs at the end of the first item range (second visits) and of the last one (second / third visits)
    'visit36k': dict(n=36000, isolated=0, hub_in={4200: 65, 4300: 320, 35750: 1000, 35800: 320, 35850: 65}, hub_out={},
                     background=50000, seed=3601),
    'visit70k': dict(n=70000, isolated=0, hub_in={5000: 65, 8600: 320, 69750: 1000, 69800: 320, 69850: 65}, hub_out={},
                     background=90000, seed=7001),
}
EXPLICIT_LOOPS = (3, 100, 1200, 1300, 2500)              # dropped by build_csr, which appends one loop per node


def dominated_hubs(name):
    """The listed hub rows with more than two in-edges: the rows the dominant_* regimes apply to."""
    return [v for v, k in SPEC[name]['hub_in'].items() if k > 2]


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> namespace(n, ei [2, E], head {hub: source}, tail {hub: source}).  Every listed hub with more than two in-edges has one
    source of its own below every other node id (`head`, the row's first CSR slot) and one above (`tail`, its last): nodes
    with that single out-edge, so that raising their logit touches no other row.  In-edges of a hub come from distinct
    sources, the first three of them twice (multi-edges); the same for the targets of the out-degree hubs.  The background
    (random edges, the first 50 twice) touches neither the hubs nor the isolated nodes at the end."""
    s = SPEC[name]
    n, g = s['n'], torch.Generator().manual_seed(s['seed'])
    active = n - s['isolated']
    dom = dominated_hubs(name)
    head = {v: i for i, v in enumerate(dom)}
    tail = {v: active - len(dom) + i for i, v in enumerate(dom)}
    special = set(s['hub_in']) | set(s['hub_out']) | set(head.values()) | set(tail.values())
    assert len(special) == len(s['hub_in']) + len(s['hub_out']) + 2 * len(dom)
    free_mask = torch.ones(active, dtype=torch.bool)
    free_mask[list(special)] = False
    free = free_mask.nonzero().flatten()

    def distinct(k):                                    # k picks from the free nodes, the first three of them repeated
        dup = 3 if k >= 13 else 0
        pick = free[torch.randperm(free.numel(), generator=g)[:k - dup]]
        assert pick.numel() == k - dup
        return torch.cat([pick, pick[:dup]])

    parts = []
    for v, k in s['hub_in'].items():
        m = k - 1                                       # in-edges beside the loop
        if k > 2:
            src = torch.cat([torch.tensor([head[v], tail[v]]), distinct(m - 2)])
        else:
            src = distinct(m)
        parts.append(torch.stack([src, torch.full_like(src, v)]))
    for v, k in s['hub_out'].items():
        dst = distinct(k - 1)
        parts.append(torch.stack([torch.full_like(dst, v), dst]))
    rnd = free[torch.randint(0, free.numel(), (2, s['background']), generator=g)]
    parts += [rnd, rnd[:, :50]]
    if name == 'hub':
        parts.append(torch.tensor(EXPLICIT_LOOPS).expand(2, -1))
    return types.SimpleNamespace(n=n, ei=torch.cat(parts, 1).contiguous(), head=head, tail=tail)


@functools.lru_cache(maxsize=None)
def layout(name):
    """build_csr(ei, n, 'gat') on the host (it lays the graph out there; the GPU module checks that the device build gives the
    same arrays) -> namespace(gr, rows, col, deg, out_deg): the target and source of every CSR slot as int64."""
    from gnndelete_amd.graph import build_csr
    gph = graph(name)
    gr = build_csr(gph.ei, gph.n, 'gat')
    deg = (gr.rowptr[1:] - gr.rowptr[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(gph.n), deg)
    return types.SimpleNamespace(gr=gr, rows=rows, col=gr.col.long(), deg=deg, out_deg=(gr.rowptr_t[1:] - gr.rowptr_t[:-1]).long())


def edge_slot(name, hub, which):
    """CSR slot of the hub row's last ('tail') / first ('head') in-edge that is not its own loop."""
    lay = layout(name)
    lo, hi = int(lay.gr.rowptr[hub]), int(lay.gr.rowptr[hub + 1])
    slots = [k for k in (range(hi - 1, lo - 1, -1) if which == 'tail' else range(lo, hi)) if int(lay.col[k]) != hub]
    return slots[0]


# ---------------------------------------------------------------------------------------------------------------------
# logits and features
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def logits(name, regime):
    """-> (a_src, a_dst) fp32 [n] on the 2^-10 grid."""
    n = SPEC[name]['n']
    g = torch.Generator().manual_seed(SPEC[name]['seed'] + 17)
    a_src, a_dst = (torch.round(torch.randn(n, generator=g) * GRID) / GRID for _ in range(2))
    if regime == 'wide':                                 # spans of +-150 inside a row: most weights underflow
        a_src = a_src * 40
    elif regime == 'negative':                           # every logit on the slope branch; exp of the unshifted logit is 0
        a_dst = a_dst - 600
    elif regime == 'zero':                               # every logit exactly 0: alpha = 1 / deg, leaky' at 0 = the slope
        a_src, a_dst = torch.full((n,), 7.25), torch.full((n,), -7.25)
    elif regime in ('dominant_tail', 'dominant_head'):   # the row maximum sits in the last / first piece, 60 above the rest
        which = regime.split('_')[1]
        for hub in dominated_hubs(name):
            a_src[int(layout(name).col[edge_slot(name, hub, which)])] += 60
    else:
        assert regime == 'randn'
    return a_src.contiguous(), a_dst.contiguous()


@functools.lru_cache(maxsize=None)
def case(name, d):
    """fp32 (h, dy, bias, att_src, att_dst) at width d.  Column k of h and of dy carries one random sign s_k: h = |randn| s,
    dy = |randn| s.  Entries, y and dh have both signs, but every product dy_ik h_jk is >= 0, so |<dy_i, h_j>| IS the sum of
    the magnitudes the dot product adds up and the score-gradient scales of reference() see all of them.  (With independent
    signs <dy, h> cancels inside itself: alpha (|<dy, h>| + |t|) can then be 1e-3 of the d terms behind it, and fp32 - the
    restatement too - sits at up to 1e-4 of that scale on the worst of 20,000 slots, by the luck of one rounding.)"""
    n = SPEC[name]['n']
    g = torch.Generator().manual_seed(SPEC[name]['seed'] + 1000 + d)
    sign = torch.where(torch.rand(d, generator=g) < 0.5, -1.0, 1.0)
    return dict(h=torch.randn(n, d, generator=g).abs() * sign, dy=torch.randn(n, d, generator=g).abs() * sign,
                bias=torch.randn(d, generator=g) + 0.25,
                att_src=torch.randn(d, generator=g) / d ** 0.5, att_dst=torch.randn(d, generator=g) / d ** 0.5)


@functools.lru_cache(maxsize=None)
def row_subset(name):
    """Section D: the 5,000-, 320-, 257- and 64-row hubs plus a third of the other rows -> sorted int64 ids."""
    n = SPEC[name]['n']
    g = torch.Generator().manual_seed(SPEC[name]['seed'] + 5)
    keep = torch.rand(n, generator=g) < 1 / 3
    keep[list(SPEC[name]['hub_in']) + list(SPEC[name]['hub_out'])] = False
    keep[[1200, 1000, 900, 400, 1400, 1600]] = True              # ... and the sources of 257 and 1,000 out-edges
    return keep.nonzero().flatten()


SUBSET_RANGE = (400, 1001)          # row_range cutting through the hub ids: 400 (64 in-edges) is the first row, 1000 (320) the last


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def _run(name, regime, d, dtype, dy_rows=None):
    """GATConv's aggregation over the CSR slots in `dtype` with pyg_semantics' softmax and scatter, and autograd: y without
    the bias, the row statistics, alpha and the gradient of the pre-activation score per slot, the message-path dh, da_src,
    da_dst.  dy_rows: the upstream gradient is zero outside these rows (what a plan over a row subset computes)."""
    lay, c = layout(name), case(name, d)
    n, rows, col = SPEC[name]['n'], lay.rows, lay.col
    a_s, a_d = (t.to(dtype).clone().requires_grad_() for t in logits(name, regime))
    h = c['h'].to(dtype).clone().requires_grad_()
    dy = c['dy'].to(dtype)
    if dy_rows is not None:
        keep = torch.zeros(n, dtype=torch.bool)
        keep[dy_rows] = True
        dy = dy * keep[:, None]
    s = a_s[col] + a_d[rows]
    s.retain_grad()
    e = F.leaky_relu(s, SLOPE)
    alpha = pyg.segment_softmax(e, rows, n)
    y = pyg.scatter_rows(h[col] * alpha[:, None], rows, n)
    y.backward(dy)
    ed = e.detach()
    rowmax = torch.full((n,), -float('inf'), dtype=dtype).scatter_reduce(0, rows, ed, reduce='amax', include_self=True)
    rowsum = torch.zeros(n, dtype=dtype).index_add(0, rows, (ed - rowmax[rows]).exp())
    return dict(y=y.detach(), rowmax=rowmax, rowsum=rowsum, alpha=alpha.detach(), de=s.grad, dh=h.grad, da_src=a_s.grad,
                da_dst=a_d.grad, s=s.detach(), dy=dy)


@functools.lru_cache(maxsize=None)
def reference(name, regime, d, subset=False):
    """The fp64 reference with the scale of every measure (the sum of the magnitudes that the row or slot adds up):
       y_scale / y_scale_bias   || sum_j alpha_ij |h_j| (+ |b|) ||_2
       dh_scale                 || sum_i alpha_ij |dy_i| ||_2
       de_scale (per slot)      alpha_ij (|<dy_i, h_j>| + |t_i|),  t_i = sum_j alpha_ij <dy_i, h_j>
       da_dst_scale / da_src_scale   de_scale summed over the row's in-edges / the node's out-edges
    each floored at 1e-30 x its largest value.  subset: dy is zero outside row_subset(name)."""
    lay, c = layout(name), case(name, d)
    n, rows, col = SPEC[name]['n'], lay.rows, lay.col
    r = _run(name, regime, d, torch.float64, row_subset(name) if subset else None)
    h, dy, b = c['h'].double(), r.pop('dy'), c['bias'].double()
    alpha = r['alpha']
    floor = lambda t: t.clamp_min(SCALE_FLOOR * float(t.max()))
    y_abs = pyg.scatter_rows(h.abs()[col] * alpha[:, None], rows, n)
    r['y_scale'], r['y_scale_bias'] = floor(y_abs.norm(dim=1)), floor((y_abs + b.abs()).norm(dim=1))
    del y_abs
    r['dh_scale'] = floor(pyg.scatter_rows(dy.abs()[rows] * alpha[:, None], col, n).norm(dim=1))
    p = (dy[rows] * h[col]).sum(1)
    t = torch.zeros(n, dtype=torch.float64).index_add(0, rows, alpha * p)
    mag = alpha * (p.abs() + t.abs()[rows])
    r['de_scale'] = floor(mag)
    r['da_dst_scale'] = floor(torch.zeros(n, dtype=torch.float64).index_add(0, rows, mag))
    r['da_src_scale'] = floor(torch.zeros(n, dtype=torch.float64).index_add(0, col, mag))
    r['rowmax_ulp'] = (torch.nextafter(r['rowmax'].float().abs(), torch.tensor(float('inf'))) - r['rowmax'].float().abs()).double()
    r['span'] = float(r['s'].max() - r['s'].min())
    return r


def errors(got, name, regime, d, bias=False, subset=False):
    """Per-row (per-slot for alpha and de) error of every tensor in `got` against the fp64 reference, under the measures of
    reference().  got: any of y, rowmax, rowsum, alpha, de, dh, da_src, da_dst, dh_full (the batch step's whole input
    gradient dh + da_src (x) att_src + da_dst (x) att_dst); y includes the bias when `bias`.  rowmax comes out in fp32 ulps."""
    ref, c = reference(name, regime, d, subset), case(name, d)
    out = {}
    for k, v in got.items():
        v = v.detach().cpu().double()
        if k == 'y':
            want = ref['y'] + c['bias'].double() if bias else ref['y']
            out[k] = (v - want).norm(dim=1) / ref['y_scale_bias' if bias else 'y_scale']
        elif k == 'dh':
            out[k] = (v - ref['dh']).norm(dim=1) / ref['dh_scale']
        elif k == 'dh_full':
            us, ud = c['att_src'].double(), c['att_dst'].double()
            want = ref['dh'] + ref['da_src'][:, None] * us + ref['da_dst'][:, None] * ud
            scale = ref['dh_scale'] + ref['da_src_scale'] * float(us.norm()) + ref['da_dst_scale'] * float(ud.norm())
            out[k] = (v - want).norm(dim=1) / scale
        elif k == 'rowmax':
            out[k] = (v - ref['rowmax']).abs() / ref['rowmax_ulp']
        elif k == 'rowsum':
            out[k] = (v - ref['rowsum']).abs() / ref['rowsum']
        elif k == 'alpha':
            out[k] = (v - ref['alpha']).abs()
        else:
            out[k] = (v - ref[k]).abs() / ref[k + '_scale']
    return out


def _restatement(name, regime, d, subset):
    r = _run(name, regime, d, torch.float32, row_subset(name) if subset else None)
    c = case(name, d)
    r['dh_full'] = r['dh'] + r['da_src'][:, None] * c['att_src'] + r['da_dst'][:, None] * c['att_dst']
    r['y_bias'] = r['y'] + c['bias']
    return r


@functools.lru_cache(maxsize=None)
def restatement_errors(name, regime, d, subset=False):
    """Largest error of the SAME formula in torch.float32 on the host, per quantity: what the kernels' bounds are taken from
    ('y_bias': y with the bias under its own scale; 'finite': every fp32 result is finite)."""
    r = _restatement(name, regime, d, subset)
    keys = ('y', 'rowmax', 'rowsum', 'alpha', 'de', 'dh', 'da_src', 'da_dst', 'dh_full')
    out = {k: float(v.max()) for k, v in errors({k: r[k] for k in keys}, name, regime, d, False, subset).items()}
    out['y_bias'] = float(errors({'y': r['y_bias']}, name, regime, d, True, subset)['y'].max())
    out['finite'] = all(bool(torch.isfinite(r[k]).all()) for k in keys)
    return out


def bounds(name, regime, d, subset=False):
    """max(8 x the restatement's error, 2^-22) per quantity; rowmax: two fp32 ulps of the fp64 row maximum."""
    r = restatement_errors(name, regime, d, subset)
    out = {k: max(SOFTMAX_FACTOR * v, SOFTMAX_FLOOR) for k, v in r.items() if k not in ('rowmax', 'finite')}
    out['rowmax'] = ROWMAX_ULPS
    return out


# ---------------------------------------------------------------------------------------------------------------------
# visits of the persistent item kernels (gat_items_fwd_kernel / gat_items_bwd_dalpha_kernel)
# ---------------------------------------------------------------------------------------------------------------------
GRID_CAP, XCDS = 8192, 8


def visit_of_items(n_items, xcd_bounds=None):
    """The launch arithmetic restated: min(ceil(n_items / 4), 8192) blocks rounded up to 8, stride = blocks / 8 * 4 waves per
    XCD, XCD x sweeps [x per, (x + 1) per) with per = ceil(n_items / 8), or [bounds[x], bounds[x + 1]) of a range table; its
    wave w visits items first + w, first + w + stride, ...  -> int64 [n_items]: on which of its wave's visits an item is served."""
    nblk = min((n_items + 3) // 4, GRID_CAP)
    nblk = (nblk + XCDS - 1) // XCDS * XCDS
    stride = nblk // XCDS * 4
    idx = torch.arange(n_items)
    if xcd_bounds is None:
        per = (n_items + XCDS - 1) // XCDS
        first = idx // per * per
    else:
        b = torch.as_tensor(xcd_bounds).long().cpu()
        assert b.numel() == XCDS + 1 and int(b[0]) == 0 and int(b[-1]) == n_items
        first = b[torch.searchsorted(b[1:].contiguous(), idx, right=True)]
    return (idx - first) // stride


def item_tables(name, form, d):
    """(item rows, visit of every item) of the forward / the piece-form backward ('pieces') or the one-launch backward
    ('onepass', rows < 0 = padding) of the whole graph at width d."""
    plan = layout(name).gr.plan
    if form == 'pieces':
        return plan.items[:, 0].long(), visit_of_items(plan.n_items)
    items, n_items, b = plan.onepass(d, multirow=1)
    return items[:, 0].long(), visit_of_items(n_items, b)


def later_visit_rows(name, form, d):
    """Sorted ids of the rows with an item that its wave serves on a second or later visit."""
    rows, visit = item_tables(name, form, d)
    sel = rows[(visit >= 1) & (rows >= 0)]
    return torch.unique(sel)
