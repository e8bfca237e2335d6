"""Shared inputs and references of the SpMM form tests (test_spmm_cases_cpu.py, test_spmm_forms_gpu.py, spmm_visits_worker.py):
ONE crafted CSR built for the edges of the plans SplitPlan hands to the aggregation kernels of csrc/spmm.hip - runs of light
rows that fill a multi-row item's 7-bit cumulative counts to exactly 64, start / continue / end it with empty rows or consist of
empty rows only, each run between two hub rows of 70 in-edges (the planner packs light rows in fixed pairs / quadruples counted
from the start of a run, and a run starts after a hub); hub rows at every count where the group members' shares change shape
(65 .. 5000), as first row, as last row behind an empty one (the nnz - 1 clamp of the index prefetch is live) and side by side -
three plans over it (every row, a row subset with gaps inside the runs, a row range whose limits fall inside runs), and the
transposed CSR of the same edges.  Everything is deterministic from seeds and drawn in fp32, only then widened.  References are
computed once per process (lru_cache) and must be left unchanged by their users.

    y[i] = sum_{k in row i} w_k x[col_k] + self_coef * x_self[i] + bias

Two kinds of data.  'int': x, x_self, bias integer-valued in [-8, 8], w in {0.25, 0.5, 1, 2} or 1, self_coef in {0, 1, 0.5}: every
term is a multiple of 2^-3 and every partial sum stays below 2^17 (5000 edges x 2 x 8 = 80,000), so every fp32 sum is exact in
any order, with or without fma, on the vector and on the matrix pipe - every form has to give the fp64 reference BIT FOR BIT, and
one dropped, doubled or misattributed edge changes an element.  'float': N(0, 1) data with symmetric-normalisation weights
1 / sqrt((deg_i + 1)(deg_j + 1)) formed in fp32 ('gcn': what gcn_norm gives an edge once the self term stands for the self loop)
or rand + 0.25 ('rand'), held per ELEMENT to

    |y - ref64| <= gamma_k S,   k = in-degree + 2,  gamma_k = k u / (1 - k u),  u = 2^-24,
    S = sum |w| |x| + |self_coef| |x_self| + |b|   (fp64)

- every product enters through one fma, an add of an exact zero is exact, so no path from a leaf to the stored value has more
than k roundings in any form (lane-group chains + xor tree + member / piece sums + self term + bias).  S = 0: equality."""
import functools
import operator

import torch

N = 2600
DMAX = 1028                                        # the widest row of any test; narrower widths take the first d columns
SEP = 70                                           # the hub row in front of and behind every crafted run
RUNS = {'64_0_0_0': [64, 0, 0, 0], '0_0_0_64': [0, 0, 0, 64], '0_0_0_0': [0, 0, 0, 0], '16x4': [16, 16, 16, 16],
        '16_16_16_17': [16, 16, 16, 17], '1_62_1': [1, 62, 1], '32_32': [32, 32], '32_33': [32, 33], '0_64': [0, 64], '64_0': [64, 0]}
LATE_RUNS = {'late_16x4': [16, 16, 16, 16], 'late_1_62_1': [1, 62, 1]}       # a second block: the row range ends inside it
BLOCK0, BLOCK1 = 40, 2400                          # first rows of the two blocks of crafted runs
HUBS = {0: 65, 300: 128, 500: 129, 700: 192, 701: 193, 900: 256, 901: 257, 1100: 320, 1300: 321, 1500: 1025, 1900: 5000, N - 1: 130}
BIG = (1900, 1500, 1300, 1100, 901)                # the rows above 4 pieces (256 in-edges), heaviest first
OPTIONS = ((True, True, 0.0, None), (False, False, 1.0, 'xs'), (True, True, 0.5, 'xs'), (False, True, 1.0, 'x'),
           (False, False, 1.0, 'x'), (True, True, 0.5, 'x'))
#          (weighted, bias, self_coef, where the self term is read from); float data: option 0 runs 'gcn' weights, 2 and 5 'rand';
#          4 and 5 = 1 and 2 for the plain entry, which has no separate x_self
PLAIN_OPTIONS = (0, 4, 5, 3)
XCDS, GRID_CAP, CHUNK = 8, 8192, 64
U = 2.0 ** -24


def _layout():
    """-> (degree vector, {run name: first row})."""
    g = torch.Generator().manual_seed(2600)
    deg = torch.randint(0, 9, (N,), generator=g)
    where = {}
    for block, runs in ((BLOCK0, RUNS), (BLOCK1, LATE_RUNS)):
        r = block
        for name, degs in runs.items():
            deg[r] = SEP
            where[name] = r + 1
            deg[r + 1:r + 1 + len(degs)] = torch.tensor(degs)
            r += 1 + len(degs)
        deg[r] = SEP
    for row, k in HUBS.items():
        deg[row] = k
    deg[N - 2] = 0
    return deg, where


DEG, RUN_START = _layout()


def _csr(src, dst):
    order = torch.argsort(dst * N + src, stable=True)
    rowptr = torch.zeros(N + 1, dtype=torch.long)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=N), 0)
    return rowptr.to(torch.int32), src[order].to(torch.int32).contiguous(), order


@functools.lru_cache(maxsize=None)
def graph():
    """{'fwd': (rowptr, col), 'bwd': (rowptr_t, col_t), 'perm_t': forward entry of every transposed entry}, int32 on the host; rows
    sorted by (target, source) as build_csr sorts them.  Sources are drawn from every row, hubs and empty rows included."""
    g = torch.Generator().manual_seed(2601)
    dst = torch.repeat_interleave(torch.arange(N), DEG)
    src = torch.randint(0, N, (int(DEG.sum()),), generator=g)
    rowptr, col, order = _csr(src, dst)
    rowptr_t, col_t, order_t = _csr(dst, src)
    pos = torch.empty_like(order)
    pos[order] = torch.arange(order.numel())
    assert torch.equal((rowptr[1:] - rowptr[:-1]).long(), DEG)
    return {'fwd': (rowptr, col), 'bwd': (rowptr_t, col_t), 'perm_t': pos[order_t]}


def degrees(direction):
    rp = graph()[direction][0].long()
    return rp[1:] - rp[:-1]


def row_of_entry(direction):
    return torch.repeat_interleave(torch.arange(N), degrees(direction))


PLANS = ('full', 'subset', 'range')


@functools.lru_cache(maxsize=None)
def plan_rows(name):
    """Sorted row ids of a plan (the same ids in both directions)."""
    if name == 'full':
        return torch.arange(N)
    if name == 'range':                              # from the second row of '16x4' up to the first two rows of 'late_16x4'
        return torch.arange(RUN_START['16x4'] + 1, RUN_START['late_16x4'] + 2)
    g = torch.Generator().manual_seed(2602)
    keep = torch.rand(N, generator=g) < 0.6
    keep[BLOCK0:BLOCK0 + 60] = False                 # the first block: only what is named here
    r = RUN_START
    for row in (r['16x4'], r['16x4'] + 1, r['16x4'] + 3,                     # a pair, then a single
                r['64_0_0_0'] + 1, r['64_0_0_0'] + 2, r['64_0_0_0'] + 3,     # three empty rows: an item without an edge
                r['0_0_0_64'], r['0_0_0_64'] + 3,                            # two singles
                r['1_62_1'] - 1, r['1_62_1'], r['1_62_1'] + 1,               # a hub, then 1 + 62
                r['64_0'], r['64_0'] + 1, r['64_0'] + 2,                     # 64 + 0, then the hub behind them
                0, N - 2, N - 1, 700, 701, 900, 1500, 1900):                 # hubs (first, last, side by side, > 4 pieces)
        keep[row] = True
    for row in (300, 500, 901, 1100, 1300):
        keep[row] = False
    return keep.nonzero().flatten()


def split_plan(name, direction, device='cpu'):
    """A SplitPlan of graph()[direction] over plan_rows(name) (not cached: a plan keeps device buffers)."""
    from gnndelete_amd.graph import SplitPlan
    rowptr = graph()[direction][0].to(device)
    if name == 'full':
        return SplitPlan(rowptr)
    if name == 'range':
        rows = plan_rows(name)
        return SplitPlan(rowptr, row_range=(int(rows[0]), int(rows[-1]) + 1))
    return SplitPlan(rowptr, rows=plan_rows(name).to(device))


# ---------------------------------------------------------------------------------------------------------------------
# data and references
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def data(kind):
    """fp32 {'x', 'xs' [N, DMAX], 'b' [DMAX], 'val': {name: [nnz] in forward entry order}}."""
    nnz = int(DEG.sum())
    if kind == 'int':
        g = torch.Generator().manual_seed(2603)
        draw = lambda *s: torch.randint(-8, 9, s, generator=g).float()
        val = {'w': torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (nnz,), generator=g)]}
        return {'x': draw(N, DMAX), 'xs': draw(N, DMAX), 'b': draw(DMAX), 'val': val}
    assert kind == 'float'
    g = torch.Generator().manual_seed(2604)
    x, xs, b = torch.randn(N, DMAX, generator=g), torch.randn(N, DMAX, generator=g), torch.randn(DMAX, generator=g)
    rowptr, col = graph()['fwd']
    inv = 1.0 / torch.sqrt(DEG.float() + 1.0)
    gcn = inv[row_of_entry('fwd')] * inv[col.long()]
    return {'x': x, 'xs': xs, 'b': b, 'val': {'gcn': gcn, 'rand': torch.rand(nnz, generator=g) + 0.25}}


def val_name(kind, option):
    """Which weights option `option` runs on data of a kind (None: unweighted)."""
    if not OPTIONS[option][0]:
        return None
    return 'w' if kind == 'int' else ('gcn' if option == 0 else 'rand')


def edge_values(kind, name, direction):
    """fp32 [nnz] in the entry order of a direction, None for unweighted."""
    if name is None:
        return None
    v = data(kind)['val'][name]
    return v if direction == 'fwd' else v[graph()['perm_t']].contiguous()


def aggregate(rowptr, col, val, x, dtype, order=None):
    """sum_k w_k x[col_k] per row by a sparse index_add_ in `dtype` (order: a permutation of the entries - another summation
    order)."""
    rp = rowptr.long()
    rows = torch.repeat_interleave(torch.arange(rp.numel() - 1), rp[1:] - rp[:-1])
    c = col.long()
    w = torch.ones(c.numel(), dtype=dtype) if val is None else val.to(dtype)
    if order is not None:
        rows, c, w = rows[order], c[order], w[order]
    return torch.zeros(rp.numel() - 1, x.shape[1], dtype=dtype).index_add_(0, rows, w[:, None] * x.to(dtype)[c])


@functools.lru_cache(maxsize=None)
def _ax(kind, name, direction, absolute):
    rowptr, col = graph()[direction]
    v, x = edge_values(kind, name, direction), data(kind)['x']
    return aggregate(rowptr, col, v.abs() if (absolute and v is not None) else v, x.abs() if absolute else x, torch.float64)


@functools.lru_cache(maxsize=None)
def reference(kind, option, direction):
    """fp64 [N, DMAX] of an option on every row."""
    weighted, with_bias, coef, src = OPTIONS[option]
    c = data(kind)
    y = _ax(kind, val_name(kind, option), direction, False).clone()
    if coef != 0.0:
        y += coef * c[src].double()
    if with_bias:
        y += c['b'].double()
    return y


@functools.lru_cache(maxsize=None)
def scale(option, direction):
    """S of the float data: fp64 [N, DMAX]."""
    weighted, with_bias, coef, src = OPTIONS[option]
    c = data('float')
    s = _ax('float', val_name('float', option), direction, True).clone()
    if coef != 0.0:
        s += abs(coef) * c[src].double().abs()
    if with_bias:
        s += c['b'].double().abs()
    return s


def gamma(k):
    k = torch.as_tensor(k, dtype=torch.float64)
    return k * U / (1.0 - k * U)


@functools.lru_cache(maxsize=None)
def bound(option, direction):
    """gamma_k S per element, k = in-degree + 2: fp64 [N, DMAX]."""
    return gamma(degrees(direction) + 2)[:, None] * scale(option, direction)


def error_ratio(got, ref, bnd):
    """max |got - ref| / bound over the elements given (same shapes); an element with bound 0 must be exact (inf otherwise)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the launch arithmetic and the item tables, restated
# ---------------------------------------------------------------------------------------------------------------------
def launch_shape(n_items, cap=GRID_CAP):
    """(blocks, waves per XCD) of launch_persist / launch_wide: min(ceil(n_items / 4), cap) blocks rounded up to 8."""
    nblk = min((n_items + 3) // 4, cap)
    nblk = (nblk + XCDS - 1) // XCDS * XCDS
    return nblk, nblk // XCDS * 4


def visit_of_items(n_items, xcd_bounds=None, cap=GRID_CAP):
    """XCD x sweeps [x per, (x + 1) per) with per = ceil(n_items / 8), or [bounds[x], bounds[x + 1]) of a range table; its wave w
    visits items first + w, first + w + stride, ...  -> int64 [n_items]: on which of its wave's visits (0 = first) an item is served."""
    stride = launch_shape(n_items, cap)[1]
    idx = torch.arange(n_items)
    if xcd_bounds is None:
        per = (n_items + XCDS - 1) // XCDS
        first = idx // per * per
    else:
        b = torch.as_tensor(xcd_bounds).long().cpu()
        assert b.numel() == XCDS + 1 and int(b[0]) == 0 and int(b[-1]) == n_items
        first = b[torch.searchsorted(b[1:].contiguous(), idx, right=True)]
    return (idx - first) // stride


def visits_per_wave(n_items, xcd_bounds, cap=GRID_CAP):
    """Visits of the busiest-to-idlest waves: [(range length, fewest visits of a wave of that XCD)] per XCD."""
    stride = launch_shape(n_items, cap)[1]
    b = torch.as_tensor(xcd_bounds).long().tolist()
    return [(b[k + 1] - b[k], (b[k + 1] - b[k]) // stride) for k in range(XCDS)]


def max_rows(d):
    """Rows per item the item kernel of width d decodes (csrc/spmm.hip MAXR): by the float4 vectors its instantiation covers."""
    d4 = d // 4
    w4 = next(w for w in (1, 2, 4, 8, 16, 32, 64, 128, 256) if d4 <= w)
    return 1 if w4 >= 32 else (2 if w4 == 16 else 4)


def decode_multi(slot, maxr, shift=7, count_from=None):
    """(rows, [b1, b2, b3]) of a multi-row slot word as spmm_persist_body reads it (fields past the rows are 'far')."""
    far = 1 << 20
    v = -slot - 16
    nr = ((v >> 21) & 3) + 1
    b1 = v & 127
    b2 = (v >> shift) & 127 if (maxr > 2 and nr > 2) else far
    b3 = (v >> (2 * shift)) & 127 if (maxr > 3 and nr > 3) else far
    return nr, [b1, b2, b3]


def item_edges(items, n_items, form, d=None, tags=None):
    """Which row every covered CSR entry is summed into: -> (entries int64 [m], rows int64 [m]) over all items, decoded as the
    kernels decode them.  form: 'onepass' (d gives MAXR), 'wide' (tags), 'pieces'."""
    ent, rows = [], []
    for row, start, end, slot in items[:n_items].tolist():
        if row < 0 or end <= start:
            continue
        e = torch.arange(start, end)
        if form == 'wide' and slot != -2:
            r = row + tags[start:end].long()
        elif form == 'onepass' and slot <= -16:
            _, b = decode_multi(slot, max_rows(d))
            j = e - start
            r = row + (j >= b[0]).long() + (j >= b[1]).long() + (j >= b[2]).long()
        else:
            r = torch.full_like(e, row)
        ent.append(e)
        rows.append(r)
    if not ent:
        return torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long)
    return torch.cat(ent), torch.cat(rows)


def run_items(items, n_items, first_row, n_rows, form='onepass', d=8):
    """The items that open inside the rows [first_row, first_row + n_rows), in table order:
    [(row - first_row, rows of the item, cumulative edge counts after its rows but the last, edges)]."""
    out = []
    for row, start, end, slot in items[:n_items].tolist():
        if not first_row <= row < first_row + n_rows or slot == -2:
            continue
        if form == 'wide':
            out.append((row - first_row, -slot - 15, None, end - start))
        elif slot <= -16:
            nr, b = decode_multi(slot, 4)
            out.append((row - first_row, nr, tuple(b[:nr - 1]), end - start))
        else:
            out.append((row - first_row, 1, (), end - start))
    return sorted(out)


def packed_rule(degs, multirow):
    """What SplitPlan.onepass makes of a run of light rows that starts an item run: fixed groups of `multirow` rows counted from
    the start, one item where a group has at least two rows and at most 64 in-edges, single rows otherwise."""
    out = []
    for k in range(0, len(degs), max(multirow, 1)):
        grp = degs[k:k + max(multirow, 1)]
        if len(grp) >= 2 and sum(grp) <= CHUNK:
            cum = [sum(grp[:q + 1]) for q in range(len(grp) - 1)]
            out.append((k, len(grp), tuple(cum), sum(grp)))
        else:
            out += [(k + q, 1, (), g) for q, g in enumerate(grp)]
    return out


def greedy_rule(degs, rows=16):
    """... and SplitPlan.onepass_wide: greedy items of up to 16 rows and 64 in-edges."""
    out, k = [], 0
    while k < len(degs):
        q, tot = k, 0
        while q < len(degs) and q - k < rows and tot + degs[q] <= CHUNK:
            tot += degs[q]
            q += 1
        q = max(q, k + 1)
        out.append((k, q - k, None, sum(degs[k:q])))
        k = q
    return out


def group_rows(items, n_items):
    """[(item index, row, [member edge counts])] of the group quadruples, in table order."""
    it = items[:n_items].tolist()
    return [(i, it[i][0], [m[2] - m[1] for m in it[i:i + 4]]) for i in range(0, n_items, 4) if it[i][3] == -2]


# ---------------------------------------------------------------------------------------------------------------------
# the item tables walked on the host
# ---------------------------------------------------------------------------------------------------------------------
def _edge_sum(col, val, x, start, end, dtype, rows=None, n_rows=1):
    """Rows [n_rows, d]: entry k of [start, end) added into row rows[k - start] (row 0 without `rows`), in entry order."""
    acc = torch.zeros(n_rows, x.shape[1], dtype=dtype)
    if end > start:
        c = col[start:end].long()
        w = torch.ones(end - start, dtype=dtype) if val is None else val[start:end].to(dtype)
        acc.index_add_(0, torch.zeros(end - start, dtype=torch.long) if rows is None else rows, w[:, None] * x[c])
    return acc


def _finish(acc, row, xs, bias, self_coef):
    if self_coef != 0.0:
        acc = acc + self_coef * xs[row]
    return acc + bias if bias is not None else acc


def _walk_group(it, i, col, val, x, dtype, mis):
    row = it[i][0]
    assert i % 4 == 0 and all(m[0] == row and m[3] == -2 for m in it[i:i + 4]), 'a group quadruple off its 4-aligned place'
    total = torch.zeros(x.shape[1], dtype=dtype)
    for _, start, end, _ in it[i:i + 4]:
        part = torch.zeros(x.shape[1], dtype=dtype)
        base = start
        while True:                                          # the member's 64-edge chunks (one, unless the row is above 256 edges)
            part = part + _edge_sum(col, val, x, base, min(base + CHUNK, end), dtype)[0]
            base += CHUNK
            if base >= end - (CHUNK if mis == 'share' else 0):
                break
        total = total + part
    return row, total


def walk_onepass(items, n_items, bounds, col, val, x, xs, bias, self_coef, y0, dtype=torch.float64, split=None, mis=None):
    """What spmm_persist_body makes of an item table at the width of x, in `dtype`: whole rows, multi-row items (rows, b1, b2, b3
    of the slot word with j >= b; MAXR rows by width), group quadruples (member shares walked in 64-edge chunks, added in member
    order, self term and bias once), padding; with `split` the piece form (pieces to scratch rows, added in slot order).  Only
    the ranges [bounds[k], bounds[k + 1]) are visited.  y0: the rows no item writes keep it.
    mis: one deliberate mis-decode - 'gt' (j > b for j >= b), 'shift' (count fields read 8 bits apart), 'share' (a member stops
    one chunk short)."""
    d = x.shape[1]
    maxr = max_rows(d)
    x, xs, y = x.to(dtype), xs.to(dtype), y0.to(dtype).clone()
    bias = None if bias is None else bias.to(dtype)
    it = items[:n_items].tolist()
    b = [0, n_items] if bounds is None else torch.as_tensor(bounds).tolist()
    scratch = {}
    for k in range(len(b) - 1):
        i = b[k]
        while i < b[k + 1]:
            row, start, end, slot = it[i]
            if slot == -2:
                assert split is None and i + 4 <= b[k + 1]
                row, total = _walk_group(it, i, col, val, x, dtype, mis)
                y[row] = _finish(total, row, xs, bias, self_coef)
                i += 4
                continue
            i += 1
            if row < 0:
                continue
            if slot >= 0:
                scratch[slot] = _edge_sum(col, val, x, start, end, dtype)[0]
            elif slot == -1:
                y[row] = _finish(_edge_sum(col, val, x, start, end, dtype)[0], row, xs, bias, self_coef)
            else:
                assert slot <= -16 and maxr > 1, 'a multi-row item at a width that carries one row per item'
                nr, bq = decode_multi(slot, maxr, shift=8 if mis == 'shift' else 7)
                j = torch.arange(end - start)
                cmp = operator.gt if mis == 'gt' else operator.ge
                r = cmp(j, bq[0]).long() + cmp(j, bq[1]).long() + cmp(j, bq[2]).long()
                acc = _edge_sum(col, val, x, start, end, dtype, rows=r.clamp(max=3), n_rows=4)
                for q in range(min(nr, maxr)):
                    y[row + q] = _finish(acc[q], row + q, xs, bias, self_coef)
    if split is not None:
        for row, slot0, n, _ in split.tolist():
            tot = torch.zeros(d, dtype=dtype)
            for s in range(slot0, slot0 + n):
                tot = tot + scratch[s]
            y[row] = _finish(tot, row, xs, bias, self_coef)
    return y


def walk_wide(items, n_items, bounds, col, val, x, xs, bias, self_coef, y0, tags, dtype=torch.float64, mis=None):
    """What spmm_wide_body makes of the wide item table: up to 16 rows per item, an edge summed into the row named by bits
    24 .. 27 of its tagged index (the source id is the low 24 bits), group quadruples as the item kernel's.
    mis: 'tag' (the row tag dropped: every edge into the item's first row), 'share'."""
    colt = col.long() | (tags.long() << 24)
    src = colt & ((1 << 24) - 1)
    local = torch.zeros_like(colt) if mis == 'tag' else colt >> 24
    x, xs, y = x.to(dtype), xs.to(dtype), y0.to(dtype).clone()
    bias = None if bias is None else bias.to(dtype)
    it = items[:n_items].tolist()
    b = torch.as_tensor(bounds).tolist()
    for k in range(XCDS):
        i = b[k]
        while i < b[k + 1]:
            row, start, end, slot = it[i]
            if slot == -2:
                row, total = _walk_group(it, i, src, val, x, dtype, mis)
                y[row] = _finish(total, row, xs, bias, self_coef)
                i += 4
                continue
            i += 1
            nr = -slot - 15
            if nr <= 0:
                continue
            acc = _edge_sum(src, val, x, start, end, dtype, rows=local[start:end], n_rows=16)
            for q in range(nr):
                y[row + q] = _finish(acc[q], row + q, xs, bias, self_coef)
    return y


def operands(kind, option, direction, d):
    """(col, val, x, xs, bias, self_coef) of an option at width d on the host (xs = x where the self term is read from x)."""
    weighted, with_bias, coef, src = OPTIONS[option]
    c = data(kind)
    x = c['x'][:, :d].contiguous()
    xs = x if src in (None, 'x') else c['xs'][:, :d].contiguous()
    return (graph()[direction][1], edge_values(kind, val_name(kind, option), direction), x, xs,
            c['b'][:d].contiguous() if with_bias else None, coef)


# ---------------------------------------------------------------------------------------------------------------------
# device copies and the check every launch is held to (GPU tests and the later-visits worker)
# ---------------------------------------------------------------------------------------------------------------------
SENTINEL = 7.0
PAD = 16                                           # y is launched at pitch d + PAD: the pad columns keep the sentinel


@functools.lru_cache(maxsize=None)
def dev_graph(direction):
    rowptr, col = graph()[direction]
    return rowptr.cuda(), col.cuda()


@functools.lru_cache(maxsize=None)
def dev_values(kind, name, direction):
    v = edge_values(kind, name, direction)
    return None if v is None else v.cuda()


@functools.lru_cache(maxsize=None)
def dev_rows(kind, which, d):
    """x / xs [N, d] (contiguous) or b [d] on the device."""
    t = data(kind)[which]
    return (t[:d] if t.dim() == 1 else t[:, :d]).contiguous().cuda()


@functools.lru_cache(maxsize=None)
def dev_reference(kind, option, direction):
    return reference(kind, option, direction).cuda(), (bound(option, direction).cuda() if kind == 'float' else None)


@functools.lru_cache(maxsize=None)
def dev_plan_rows(name):
    rows = plan_rows(name).cuda()
    outside = torch.ones(N, dtype=torch.bool, device='cuda')
    outside[rows] = False
    return rows, outside


def hold(launch, d, plan_name, direction, options=(0, 1, 2, 3), kinds=('int', 'float'), place=None, tag=''):
    """Run launch(val, x, bias, self_coef, y, x_self) - device tensors; x_self None where the self term is read from x, y a [N, d]
    view at pitch d + PAD - for every option on both kinds of data and hold it: integer data bit for bit to the fp64 reference on
    the plan's rows, float data under gamma_k S per element, every row outside the plan and every pad column the sentinel.
    place(t): where x / x_self live (another pitch or base pointer, same values).  -> the largest error / bound ratio."""
    rows, outside = dev_plan_rows(plan_name)
    worst = 0.0
    for option in options:
        weighted, with_bias, coef, src = OPTIONS[option]
        for kind in kinds:
            x = dev_rows(kind, 'x', d)
            xs = dev_rows(kind, 'xs', d) if src == 'xs' else None
            if place is not None:
                x, xs = place(x), (None if xs is None else place(xs))
            yb = torch.full((N, d + PAD), SENTINEL, device='cuda')
            launch(dev_values(kind, val_name(kind, option), direction), x, dev_rows(kind, 'b', d) if with_bias else None, coef, yb[:, :d], xs)
            ref, bnd = dev_reference(kind, option, direction)
            y = yb[:, :d]
            where = (tag, d, plan_name, direction, option, kind)
            if kind == 'int':
                bad = (y[rows].double() != ref[rows, :d]).any(1).nonzero().flatten()
                assert bad.numel() == 0, (where, 'rows that differ from the exact sum', rows[bad][:8].tolist())
            else:
                ratio = error_ratio(y[rows], ref[rows, :d], bnd[rows, :d])
                assert ratio <= 1.0, (where, 'error / (gamma_k S)', ratio)
                worst = max(worst, ratio)
            assert bool((yb[:, d:] == SENTINEL).all()), (where, 'a pad column was written')
            assert bool((y[outside] == SENTINEL).all()), (where, 'a row outside the plan was written')
    return worst
