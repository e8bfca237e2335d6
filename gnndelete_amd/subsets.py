"""The validation subsets drawn on the device (--device_subsets; csrc/rankeval.hip: gd_subset_draw, gd_subset_rank_metrics_drawn).

A validation of an unlearning request ranks the Df scores against 500 random |Df|-subsets of the Dr scores.  Upstream draws each
subset as torch.randperm(|Dr|)[:|Df|] (base.py:530-539 in the knowledge-graph trainer, fresh per evaluation; base.py:263-268 in
the link trainer, once per request): 500 permutations of the WHOLE pool to keep |Df| entries of each, and a [500, |Df|] int64
index matrix that the rank kernel reads once.  Here a subset is the first k outputs of a keyed permutation of [0, m) - a pure
function of (seed, draw, b, j, m) in integer operations, with no generator state - so the rank kernel computes member j of
subset b where it used to read idx[b, j], and nothing is drawn or stored ahead of it.  The stream is NOT upstream's: the same
statistic (a mean over 500 uniformly random k-subsets) from other subsets.

The stream, which reference_draw below restates in numpy bit for bit (it is the kernels' test oracle), with mix64 the splitmix64
finaliser (csrc/common.h) and fmix32 the murmur3 32-bit finaliser:

    bits = max(6, bit_length(m - 1)) rounded up to even;  h = bits / 2;  mask = 2^h - 1      (32 <= m < 2^31: bits <= 32, h <= 16)
    base = mix64(seed ^ mix64(draw));   kb = mix64(base + b);   key[r] = low 32 bits of mix64(kb + r),  r = 0 .. 11
    P(v):  L = v >> h, R = v & mask;  twelve times (L, R) <- (R, L ^ (fmix32(R ^ key[r]) & mask));  return (L << h) | R
    e(b, j) = the first of P(j), P(P(j)), ... that is below m                                  (cycle walking; uint32 throughout)

P is a balanced Feistel network: a bijection of [0, 2^bits) whatever the round function.  The walk from j < m stays on j's cycle
of P and that cycle returns to j, which is below m, so the walk ends; j -> e(b, j) is the permutation P induces on [0, m), so
the k members of a subset are distinct - the precondition rankeval.subset_auc_ap states for its index rows.  2^bits < 4 m, so a
member takes fewer than 4 applications on average.  Below 6 bits the domain is too narrow for the rounds to mix (a pool of 5 in
a 4-bit domain stays biased at twelve rounds), hence the floor of 6 bits and of m >= 32: a smaller pool keeps upstream's draw."""
import numpy as np
import torch

from .negatives import mix64

ROUNDS = 12         # part of the stream, not a tuning knob
MIN_POOL = 32

_M64 = 0xFFFFFFFFFFFFFFFF
_CHUNK = 1 << 22    # members per pass of reference_draw


def device_subsets_unsupported(m, k):
    """None when the subset stream draws k-subsets of a pool of m, else the reason (one line)."""
    m, k = int(m), int(k)
    if m < MIN_POOL:
        return f'a pool of {m} scores (the subset stream takes {MIN_POOL} and more)'
    if m >= 1 << 31:
        return f'a pool of {m} scores (below 2^31)'
    if k < 1:
        return f'subsets of {k} positives (at least one)'
    if k > m:
        return f'subsets of {k} positives from a pool of {m}'
    return None


def half_bits(m):
    """h of the stream: half the width of the permutation's domain."""
    return (max(6, (int(m) - 1).bit_length()) + 1) // 2


def fmix32(x):
    """The murmur3 32-bit finaliser on a numpy uint32 array, wrapping."""
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85ebca6b)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xc2b2ae35)
    return x ^ (x >> np.uint32(16))


def subset_keys(seed, draw, n_sub, first=0):
    """key[b, r] of the subsets first .. first + n_sub - 1: uint32 [n_sub, ROUNDS]."""
    with np.errstate(over='ignore'):
        base = mix64(np.uint64(int(seed) & _M64) ^ mix64(np.uint64(int(draw) & _M64)))
        kb = mix64(base + np.arange(int(first), int(first) + int(n_sub), dtype=np.uint64))
        return (mix64(kb[:, None] + np.arange(ROUNDS, dtype=np.uint64)[None]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def reference_draw(seed, draw, n_sub, k, m):
    """gd_subset_draw on the CPU -> int64 [n_sub, k] numpy array: row b holds e(b, 0 .. k - 1).  Vectorised over the members:
    every pass applies P to the members still at or above m."""
    n_sub, k, m = int(n_sub), int(k), int(m)
    reason = device_subsets_unsupported(m, k)
    if reason is not None:
        raise ValueError(f'reference_draw: {reason}')
    if n_sub < 0 or n_sub >= 1 << 31:
        raise ValueError(f'reference_draw: {n_sub} subsets (0 to 2^31 - 1)')
    h = np.uint32(half_bits(m))
    mask = np.uint32((1 << int(h)) - 1)
    out = np.empty((n_sub, k), dtype=np.int64)
    rows = max(1, _CHUNK // k)                                   # subsets per pass: the arrays of a pass stay small
    for b0 in range(0, n_sub, rows):
        n = min(rows, n_sub - b0)
        keys = subset_keys(seed, draw, n, first=b0)               # [n, ROUNDS]
        v = np.tile(np.arange(k, dtype=np.uint32), n)            # member (b, j) at b * k + j
        todo = np.arange(n * k)
        for _ in range(1 << (2 * int(h))):                       # the walk's bound; every member is done long before
            if todo.size == 0:
                break
            w, sub = v[todo], todo // k
            left, right = w >> h, w & mask
            for r in range(ROUNDS):
                left, right = right, left ^ (fmix32(right ^ keys[sub, r]) & mask)
            w = (left << h) | right
            v[todo] = w
            todo = todo[w >= np.uint32(m)]
        out[b0:b0 + n] = v.reshape(n, k)
    return out


def draw(seed, draw, n_sub, k, m, out=None, device=None):
    """gd_subset_draw on the device -> int64 [n_sub, k] (a view of `out` when given: int64 [n_sub, >= k] with unit column stride;
    columns at and beyond k are left alone).  Raises ValueError where device_subsets_unsupported gives a reason."""
    from . import _lib
    from ._lib import check, ptr, stream_ptr
    n_sub, k, m = int(n_sub), int(k), int(m)
    reason = device_subsets_unsupported(m, k)
    if reason is not None:
        raise ValueError(f'subsets.draw: {reason}')
    if out is None:
        out = torch.empty(n_sub, k, dtype=torch.int64, device=torch.device('cuda') if device is None else device)
    if (out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != n_sub or out.shape[1] < k or not out.is_cuda
            or (out.shape[1] > 1 and out.stride(1) != 1) or (n_sub > 1 and out.stride(0) < k)):
        raise ValueError(f'subsets.draw: out of shape {tuple(out.shape)} / {out.dtype}, expected int64 [{n_sub}, >= {k}] rows on the GPU')
    dev = out.device
    with torch.cuda.device(dev):
        check(_lib.lib().gd_subset_draw(int(seed) & _M64, int(draw) & _M64, n_sub, k, m, ptr(out), out.stride(0) if n_sub > 1 else max(k, out.shape[1]),
                                        stream_ptr(dev)), 'gd_subset_draw')
    return out[:, :k]
