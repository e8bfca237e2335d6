"""Negative edges drawn on the device (csrc/negatives.hip, gd_negative_edges).

The fused steps that take fresh negatives every epoch (BackboneEngine, EdgeprobEngine) are bounded by the host: a CPU randint
of 1.2 x the count, a copy, a searchsorted and a cat per epoch, and the GPU waiting for them (profiles/backbone_fused.json).
gd_negative_edges draws the same kind of pairs - negative_sampling's contract: int64 [2, n_out], no positive edge, no self
loop, uniform over the rest, duplicates possible - as a pure function of (seed, counter, slot, pos_keys, n_nodes): one launch,
no generator state, and a counter that may live on the device.  This module is the kernel's wrapper, its CPU restatement and
what the two engines share of step_device() (DeviceNegatives: the draw straight into the decoded list, the incidence list
merged from a fixed image by gd_edge_incidence_update, the counter bump - plain launches around the captured iteration);
--device_negatives switches the trainers to it.

The stream, which reference_draw below restates in numpy uint64 bit for bit (it is the kernel's test oracle):

    base = mix64(seed ^ mix64(counter))                         mix64: the splitmix64 finaliser
    try t < 64:  c = mulhi64(mix64(base + 64 * slot + t), n^2)  mulhi64: the upper half of the 128-bit product
                 accepted unless c // n == c % n or c is among pos_keys
    after 64 rejected tries:  c <- (c + 1) mod n^2, at most n^2 times, until accepted

Both need at most half of all n^2 pairs excluded (device_negatives_unsupported): a try then fails with probability <= 1/2 and
the probe, reached with probability <= 2^-64 per slot, ends because an allowed pair exists.  The draws come from a different
random stream than the host sampler's."""
import numpy as np
import torch

TRIES = 64      # the stride of a slot's counters too: part of the stream, not a tuning knob

_M32 = np.uint64(0xFFFFFFFF)


def mix64(z):
    """The splitmix64 finaliser on numpy uint64 (csrc/common.h mix64), wrapping."""
    with np.errstate(over='ignore'):
        z = np.asarray(z, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def mulhi64(a, b):
    """The upper 64 bits of a * b (numpy uint64 array, one uint64), by 32-bit halves: no partial sum overflows 64 bits."""
    a, b = np.asarray(a, dtype=np.uint64), np.uint64(b)
    a0, a1 = a & _M32, a >> np.uint64(32)
    b0, b1 = b & _M32, b >> np.uint64(32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> np.uint64(32)) + (p01 & _M32) + (p10 & _M32)
    return p11 + (p01 >> np.uint64(32)) + (p10 >> np.uint64(32)) + (mid >> np.uint64(32))


def device_negatives_unsupported(n_keys, n_nodes):
    """None when gd_negative_edges takes a graph of n_nodes nodes with n_keys distinct positive keys, else the reason (one line):
    the positives and the self loops may exclude at most half of all n_nodes^2 pairs."""
    n_keys, n = int(n_keys), int(n_nodes)
    if n < 1 or n >= 1 << 31:
        return f'{n} nodes (1 to 2^31 - 1)'
    if 2 * (n_keys + n) > n * n:
        return f'{n_keys} positive pairs and {n} self loops exclude more than half of the {n}^2 node pairs'
    return None


def _host_keys(pos_keys):
    if isinstance(pos_keys, torch.Tensor):
        pos_keys = pos_keys.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(pos_keys, dtype=np.int64).reshape(-1))


def reference_draw(pos_keys, n_nodes, seed, counter, n_out, tries=TRIES):
    """gd_negative_edges on the CPU -> int64 [2, n_out] host tensor.  pos_keys: sorted unique int64 keys (tensor or array);
    tries: the hashed tries before the linear probe (64 in the kernel; 0 leaves the probe alone, from the first try's
    candidate)."""
    keys = _host_keys(pos_keys)
    n, n_out, tries = int(n_nodes), int(n_out), int(tries)
    reason = device_negatives_unsupported(keys.size, n)
    if reason is not None:
        raise ValueError(f'reference_draw: {reason}')
    nn = np.uint64(n * n)
    un = np.uint64(n)

    def allowed(c):
        ok = (c // un) != (c % un)
        if keys.size:
            at = np.minimum(np.searchsorted(keys, c.astype(np.int64)), keys.size - 1)
            ok &= keys[at] != c.astype(np.int64)
        return ok
    with np.errstate(over='ignore'):
        base = mix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ mix64(np.uint64(int(counter) & 0xFFFFFFFFFFFFFFFF)))
        slot = np.arange(n_out, dtype=np.uint64)
        out = np.zeros(n_out, dtype=np.uint64)
        todo = np.arange(n_out)
        for t in range(max(tries, 1)):
            if todo.size == 0:
                break
            c = mulhi64(mix64(base + np.uint64(TRIES) * slot[todo] + np.uint64(t)), nn)
            out[todo] = c                                       # a rejected slot keeps its last candidate: the probe's start
            if t < tries:
                todo = todo[~allowed(c)]
        for _ in range(n * n):                                  # the probe, one pass over the pairs at the most
            if todo.size == 0:
                break
            c = out[todo] + np.uint64(1)
            c[c == nn] = np.uint64(0)
            out[todo] = c
            todo = todo[~allowed(c)]
    res = out.astype(np.int64)
    return torch.from_numpy(np.stack([res // n, res % n]))


def device_negative_edges(pos_keys, n_nodes, seed, counter, n_out, out=None):
    """gd_negative_edges on device tensors -> int64 [2, n_out] (a view of `out` when given: int64 [2, >= n_out] with unit column
    stride; columns at and beyond n_out are left alone).  pos_keys: graph_utils.positive_edge_keys on the device (None or
    empty: only self loops are excluded); counter: None (0), an int, or a one-element int64 device tensor that is read on the
    stream."""
    from . import _lib
    from ._lib import check, ptr, stream_ptr
    n_out = int(n_out)
    if out is None:
        dev = pos_keys.device if isinstance(pos_keys, torch.Tensor) else torch.device('cuda')
        out = torch.empty(2, n_out, dtype=torch.int64, device=dev)
    if out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != 2 or out.shape[1] < n_out or (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError(f'device_negative_edges: out of shape {tuple(out.shape)} / {out.dtype}, expected int64 [2, >= {n_out}] rows')
    dev = out.device
    n_keys = 0 if pos_keys is None else int(pos_keys.numel())
    if n_keys:
        if pos_keys.dtype != torch.int64 or pos_keys.device != dev or not pos_keys.is_contiguous():
            raise ValueError('device_negative_edges: pos_keys must be a contiguous int64 tensor on the output\'s device')
    if counter is not None and not isinstance(counter, torch.Tensor):
        counter = torch.tensor([int(counter)], dtype=torch.int64, device=dev)
    if counter is not None and (counter.dtype != torch.int64 or counter.device != dev or counter.numel() != 1):
        raise ValueError('device_negative_edges: counter must be one int64 on the output\'s device')
    with torch.cuda.device(dev):
        check(_lib.lib().gd_negative_edges(ptr(pos_keys) if n_keys else None, n_keys, int(n_nodes), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           ptr(counter), n_out, ptr(out), out.stride(0) if n_out else 0, stream_ptr(dev)),
              'gd_negative_edges')
    return out[:, :n_out]


def device_negatives_fallback(flag, fused, sampler_replaced, n_keys=None, n_nodes=None):
    """Why a trainer keeps the host draw under --device_negatives (one line), or None when the device draws.  flag: the fused
    flag's name; fused: whether the fused step applies to this run; sampler_replaced: the trainer module's negative_sampling
    is not graph_utils.negative_sampling (the tests' seam); n_keys / n_nodes: the excluded pairs and the graph's size."""
    if not fused:
        return f'--{flag} is missing or fell back'
    if sampler_replaced:
        return 'negative_sampling has been replaced'
    return device_negatives_unsupported(n_keys, n_nodes)


class DeviceNegatives:
    """What BackboneEngine and EdgeprobEngine share of step_device().  The host class has dec (int64 [2, n_edges], the
    first _n_fixed columns fixed), n, dev, inc_ptr / other / src_edge and _mark()."""
    _neg = None

    def enable_device_negatives(self, pos_keys, seed, counter=0):
        """Negatives from gd_negative_edges from now on (step_device): pos_keys = graph_utils.positive_edge_keys over the edges
        the draw excludes; slot i of epoch k is reference_draw(pos_keys, n, seed, counter + k, n_neg)[:, i].  Raises ValueError
        before any launch where the kernel does not take the graph; builds the image of the fixed half of the decoded list."""
        from . import _lib
        from ._lib import check, ptr, stream_ptr
        n_keys = 0 if pos_keys is None else int(pos_keys.numel())
        reason = device_negatives_unsupported(n_keys, self.n)
        if reason is not None:
            raise ValueError(f'enable_device_negatives: {reason}')
        L, dev, n = _lib.lib(), self.dev, self.n
        fixed, total = self._n_fixed, int(self.dec.shape[1])
        keys = None if not n_keys else pos_keys.to(device=dev, dtype=torch.int64).contiguous()
        image = torch.empty(L.gd_edge_incidence_fixed_bytes(n, fixed) // 8 + 1, dtype=torch.int64, device=dev)
        ws = torch.empty(L.gd_edge_incidence_update_workspace(n, total) // 8 + 1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            check(L.gd_edge_incidence_fixed(ptr(self.dec[0]), ptr(self.dec[1]), fixed, n, ptr(image), 8 * image.numel(), ptr(ws),
                                            8 * ws.numel(), stream_ptr(dev)), 'gd_edge_incidence_fixed')
        self._neg = {'keys': keys, 'seed': int(seed), 'counter': torch.tensor([int(counter)], dtype=torch.int64, device=dev),
                     'image': image, 'ws': ws}

    def _draw_and_merge(self):
        """This epoch's negatives into dec[:, fixed:] and the incidence list of the whole of dec: launches only."""
        from . import _lib
        from ._lib import check, ptr, stream_ptr
        if self._neg is None:
            raise RuntimeError('step_device: call enable_device_negatives(pos_keys, seed) first')
        st, fixed, total = self._neg, self._n_fixed, int(self.dec.shape[1])
        self._mark('start')
        device_negative_edges(st['keys'], self.n, st['seed'], st['counter'], total - fixed, out=self.dec[:, fixed:])
        self._mark('draw')
        check(_lib.lib().gd_edge_incidence_update(ptr(st['image']), ptr(self.dec[0]), ptr(self.dec[1]), fixed, total, self.n,
                                                  ptr(self.inc_ptr), ptr(self.other), ptr(self.src_edge), ptr(st['ws']),
                                                  8 * st['ws'].numel(), stream_ptr(self.dev)), 'gd_edge_incidence_update')
        self._mark('incidence')

    def _next_draw(self):
        self._neg['counter'].add_(1)        # in place, on the stream: the next epoch's draw without a word from the host
