"""The kernel forms NodeembEngine switches to from 65,536 selected rows up - the weight-stationary row GEMMs
(csrc/rows_gemm_ws.hip), the weight-stationary Del-2 kernel, the one-pass Del-1 (gd_del1_loss_wgrad_f32) and the chained Del-1
(gd_del1_chain_loss_wgrad_f32) - held to an fp64 run of the oracle on a request just above that size: 80,001 nodes,
128 -> 128 -> 64, s1 = 70,451 and s2 = 72,648 Del rows (neither a multiple of 64), 120,000 Df columns, hub rows of several
hundred edges.  The fixture-sized engine tests never reach these forms, and the collab-sized ones (test_full_size_gpu.py) reach
them with both_layerwise / mse_mean / cache_layer1=False only.

Every case builds one engine on the shared request, runs ITERS iterations from the same state with the same negatives, and
asserts
  (a) the forms: eng.forms == plan_step(eng.facts, eng.knobs), the six flags written out by hand in CASES, the row count inside
      the weight-stationary GEMM's range, the locality order on;
  (b) every iteration's train_loss within 1e-4 relative of the fp64 oracle's (test_full_size_gpu.py's bar);
  (c) z1[S1] and z2[S2] of the model's forward on the retained edges within 1e-4 rel-L2 of the fp64 oracle's (north_star); where
      the fp32 oracle ensemble (three scatter orders) itself misses 1e-4, twice the ensemble's worst distance, both printed;
  (d) both Del weights by helpers.assert_del_weights_within_fp32_spread;
  (e) a variant against the plain engine of the same (gnn, loss_type, loss_fct): loss history rtol 1e-5, weights 2e-5 rel-L2
      (test_full_size_gpu.py's bars for the affected-rows engine against the full one).
The fp64 oracle and the ensemble are computed once per (gnn, loss_type, loss_fct) and shared by every option / knob variant.
The knobs are set around the constructor only (the engine reads them there, once); the switches the LIBRARY reads once per
process (GD_DEL1_FUSED, GD_ROWS_GEMM_WS, GD_DEL2_WS) are left alone.

tests/test_engine_large_forms_cpu.py checks the request's conditions and that CASES reaches every fused-Del-1 form plan_step
can choose at this size.

Measured on an MI355X after ITERS = 6 iterations: the largest relative train_loss difference, then rel-L2 to the fp64 oracle as
`HIP / the worst member of the fp32 ensemble` (0.0e+00: a weight the update rule never steps).  All 52 cases in one run of
40 s, each engine case below 0.1 s, an oracle key 1.1 - 1.9 s once (the first, 7 s, builds the request).

  case                                  loss     z1[S1] HIP / ens   z2[S2] HIP / ens   W_D1 HIP / ens     W_D2 HIP / ens
  A/gcn/plain                           1.6e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.4e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  A/gcn/trainer                         1.7e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.4e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  A/gin/plain                           5.8e-08  1.0e-06 / 1.5e-06  1.1e-06 / 1.5e-06  9.6e-07 / 1.2e-06  7.1e-08 / 8.5e-08
  A/gin/trainer                         5.8e-08  1.0e-06 / 1.5e-06  1.1e-06 / 1.5e-06  9.6e-07 / 1.2e-06  7.1e-08 / 8.5e-08
  A/gat/plain                           2.3e-08  2.8e-07 / 2.9e-07  2.8e-07 / 2.9e-07  7.1e-08 / 1.2e-07  6.4e-08 / 6.8e-08
  A/gat/trainer                         2.3e-08  2.8e-07 / 2.9e-07  2.8e-07 / 2.9e-07  7.1e-08 / 1.2e-07  6.4e-08 / 6.8e-08
  A/sage/plain                          3.7e-08  3.9e-07 / 1.1e-06  2.3e-07 / 6.1e-07  2.7e-07 / 9.9e-07  5.9e-08 / 6.8e-08
  A/sage/trainer                        3.7e-08  1.1e-06 / 1.1e-06  6.0e-07 / 6.1e-07  1.0e-06 / 9.9e-07  6.5e-08 / 6.8e-08
  A/gcn/cache                           1.6e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.4e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  A/gcn/rows                            1.7e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.4e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  A/gcn/trainer/graph                   1.7e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.4e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  B/gcn/both_all                        2.7e-08  4.8e-07 / 2.7e-06  4.5e-07 / 2.8e-06  3.9e-07 / 2.5e-06  6.3e-08 / 1.5e-07
  B/gcn/only1                           2.9e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.5e-08 / 3.3e-07  0.0e+00 / 0.0e+00
  B/gcn/only2_layerwise                 1.7e-08  2.6e-07 / 2.7e-07  2.8e-07 / 2.9e-07  0.0e+00 / 0.0e+00  6.4e-08 / 8.3e-08
  B/gcn/only2_all                       2.0e-08  1.1e-06 / 2.7e-06  8.8e-07 / 2.0e-06  1.0e-06 / 2.6e-06  6.9e-08 / 1.1e-07
  B/gat/both_all                        1.8e-08  1.7e-06 / 9.2e-07  1.6e-06 / 8.1e-07  1.6e-06 / 9.0e-07  6.0e-08 / 6.5e-08
  B/gat/only1                           3.2e-08  2.7e-07 / 3.0e-07  2.9e-07 / 3.1e-07  7.3e-08 / 1.6e-07  0.0e+00 / 0.0e+00
  B/gat/only2_layerwise                 2.0e-08  2.6e-07 / 2.7e-07  2.7e-07 / 2.8e-07  0.0e+00 / 0.0e+00  5.5e-08 / 6.3e-08
  B/gat/only2_all                       4.2e-08  4.6e-07 / 8.4e-07  3.8e-07 / 6.7e-07  3.4e-07 / 7.1e-07  5.5e-08 / 6.8e-08
  C/gcn/kld_mean/plain                  1.3e-07  4.4e-07 / 1.2e-06  4.0e-07 / 3.3e-06  3.0e-07 / 1.0e-06  6.5e-08 / 2.7e-06
  C/gcn/kld_mean/trainer                1.3e-07  4.4e-07 / 1.2e-06  4.0e-07 / 3.3e-06  3.0e-07 / 1.0e-06  6.5e-08 / 2.7e-06
  C/gat/cosine_mean/trainer             3.4e-08  5.4e-07 / 1.8e-06  4.8e-07 / 1.4e-06  4.8e-07 / 1.6e-06  5.9e-08 / 6.6e-08
  C/gcn/cosine_sum/plain                3.0e-08  7.2e-07 / 1.5e-06  5.7e-07 / 1.2e-06  5.9e-07 / 1.6e-06  6.3e-08 / 7.9e-08
  D/gcn/plain/GD_NO_FUSED_L2            1.7e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.4e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  D/gcn/plain/GD_NO_FUSED_WGRAD2        1.9e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.4e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  D/gcn/plain/GD_DEL1_CHAIN=0           3.6e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.5e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  D/gcn/cache/GD_CACHE_SPLIT=0          1.9e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.6e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  D/gcn/plain/GD_NO_STEP_TAIL           2.8e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.6e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  D/gcn/plain/GD_NO_FUSED_LOSS1         4.5e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.6e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  D/gcn/plain/GD_NO_SPLIT               2.2e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.6e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  D/gat/plain/GD_DEL1_CHAIN=0           2.3e-08  2.8e-07 / 2.9e-07  2.8e-07 / 2.9e-07  7.1e-08 / 1.2e-07  6.4e-08 / 6.8e-08
  D/gat/plain/GD_NO_GAT_RANK1_EPILOGUE  2.3e-08  2.8e-07 / 2.9e-07  2.8e-07 / 2.9e-07  7.1e-08 / 1.2e-07  6.4e-08 / 6.8e-08
  D/gat/plain/GD_NO_GAT_DOTS            2.3e-08  2.8e-07 / 2.9e-07  2.8e-07 / 2.9e-07  7.1e-08 / 1.2e-07  6.4e-08 / 6.8e-08
  D/sage/plain/GD_NO_FUSED_L2           3.0e-08  3.9e-07 / 1.1e-06  2.3e-07 / 6.1e-07  2.7e-07 / 9.9e-07  5.9e-08 / 6.8e-08
  D/gcn/trainer/GD_DEL1_CHAIN=0         3.6e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.5e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  E/gcn/trainer/GD_NO_FUSED_L2          1.6e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.4e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  E/gcn/trainer/GD_NO_FUSED_WGRAD2      1.9e-08  2.8e-07 / 4.4e-07  2.9e-07 / 4.2e-07  7.4e-08 / 3.1e-07  6.2e-08 / 8.4e-08
  E/gin/plain/GD_NO_FUSED_L2            2.2e-08  1.0e-06 / 1.5e-06  1.1e-06 / 1.5e-06  9.6e-07 / 1.2e-06  7.1e-08 / 8.5e-08
  E/gin/plain/GD_NO_FUSED_WGRAD2        8.3e-08  1.3e-06 / 1.5e-06  1.3e-06 / 1.5e-06  1.2e-06 / 1.2e-06  7.1e-08 / 8.5e-08
  E/gin/plain/GD_DEL1_CHAIN=0           5.8e-08  1.3e-06 / 1.5e-06  1.3e-06 / 1.5e-06  1.2e-06 / 1.2e-06  7.1e-08 / 8.5e-08
  E/gin/trainer/GD_NO_FUSED_L2          2.6e-08  1.0e-06 / 1.5e-06  1.1e-06 / 1.5e-06  9.6e-07 / 1.2e-06  7.1e-08 / 8.5e-08
  E/gin/trainer/GD_NO_FUSED_WGRAD2      6.2e-08  1.3e-06 / 1.5e-06  1.3e-06 / 1.5e-06  1.2e-06 / 1.2e-06  7.1e-08 / 8.5e-08
  E/gin/trainer/GD_DEL1_CHAIN=0         6.2e-08  1.3e-06 / 1.5e-06  1.3e-06 / 1.5e-06  1.2e-06 / 1.2e-06  7.1e-08 / 8.5e-08
  E/gat/plain/GD_NO_FUSED_L2            2.3e-08  2.8e-07 / 2.9e-07  2.8e-07 / 2.9e-07  7.1e-08 / 1.2e-07  6.4e-08 / 6.8e-08
  E/gat/plain/GD_NO_FUSED_WGRAD2        2.3e-08  2.8e-07 / 2.9e-07  2.8e-07 / 2.9e-07  7.1e-08 / 1.2e-07  6.4e-08 / 6.8e-08
  E/gat/trainer/GD_NO_FUSED_L2          2.3e-08  2.8e-07 / 2.9e-07  2.8e-07 / 2.9e-07  7.2e-08 / 1.2e-07  6.4e-08 / 6.8e-08
  E/gat/trainer/GD_NO_FUSED_WGRAD2      2.3e-08  2.8e-07 / 2.9e-07  2.8e-07 / 2.9e-07  7.1e-08 / 1.2e-07  6.4e-08 / 6.8e-08
  E/gat/trainer/GD_DEL1_CHAIN=0         2.3e-08  2.8e-07 / 2.9e-07  2.8e-07 / 2.9e-07  7.1e-08 / 1.2e-07  6.4e-08 / 6.8e-08
  E/gat/trainer/GD_NO_GAT_DOTS          3.0e-08  2.8e-07 / 2.9e-07  2.8e-07 / 2.9e-07  7.1e-08 / 1.2e-07  6.4e-08 / 6.8e-08
  E/sage/plain/GD_NO_FUSED_WGRAD2       4.4e-08  3.9e-07 / 1.1e-06  2.3e-07 / 6.1e-07  2.7e-07 / 9.9e-07  5.9e-08 / 6.8e-08
  E/sage/trainer/GD_NO_FUSED_L2         3.7e-08  1.1e-06 / 1.1e-06  6.0e-07 / 6.1e-07  1.0e-06 / 9.9e-07  6.5e-08 / 6.8e-08
  E/sage/trainer/GD_NO_FUSED_WGRAD2     4.4e-08  1.1e-06 / 1.1e-06  6.0e-07 / 6.1e-07  1.0e-06 / 9.9e-07  6.5e-08 / 6.8e-08

Teeth (test_the_bars_tell_update_rules_apart): the fp64 oracles of both_layerwise and both_all after 6 iterations are 1.95e-02
apart in W_D1 (bound of (d): 5.0e-05) and 2.13e-02 in z1[S1] (bound of (c): 1.0e-04) - 390 and 213 times the bounds.
"""
import functools
from collections import namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

N, F, HID, OUT, M_EDGES, N_DF, SEED = 80001, 128, 128, 64, 320000, 60000, 3
ALPHA, LR, ITERS = 0.5, 1e-3, 6
WS_MIN_ROWS = 65536

OPTS = {'plain': {}, 'cache': dict(cache_layer1=True), 'rows': dict(affected_rows_only=True),
        'trainer': dict(cache_layer1=True, affected_rows_only=True)}        # (trainer/gnndelete_nodeemb.py: the trainer's defaults)
FLAGS = ('fuse_del1', 'chain1', 'rows_only', 'tail', 'fuse_wg2', 'split1')
Case = namedtuple('Case', 'name gnn loss_type loss_fct opts knob graph flags')


def _c(name, gnn, opts, flags, loss_type='both_layerwise', loss_fct='mse_mean', knob=None, graph=False):
    if isinstance(knob, str):
        knob = (knob, '1')
    return Case(name, gnn, loss_type, loss_fct, opts, knob, graph, dict(zip(FLAGS, map(bool, flags))))


# the flags, in the order of FLAGS: fuse_del1, chain1, rows_only, tail, fuse_wg2, split1
CASES = [
    # ---- A: default knobs, both_layerwise, mse
    _c('A/gcn/plain', 'gcn', 'plain', (1, 1, 0, 1, 1, 1)),
    _c('A/gcn/trainer', 'gcn', 'trainer', (1, 1, 1, 1, 1, 1)),
    _c('A/gin/plain', 'gin', 'plain', (1, 1, 0, 1, 1, 1)),
    _c('A/gin/trainer', 'gin', 'trainer', (1, 1, 1, 1, 1, 1)),
    _c('A/gat/plain', 'gat', 'plain', (1, 1, 0, 1, 1, 1)),
    _c('A/gat/trainer', 'gat', 'trainer', (1, 1, 1, 1, 1, 1)),
    _c('A/sage/plain', 'sage', 'plain', (1, 0, 0, 1, 1, 1)),
    _c('A/sage/trainer', 'sage', 'trainer', (1, 0, 1, 1, 1, 1)),
    _c('A/gcn/cache', 'gcn', 'cache', (1, 1, 0, 1, 1, 1)),
    _c('A/gcn/rows', 'gcn', 'rows', (1, 1, 1, 1, 1, 1)),
    _c('A/gcn/trainer/graph', 'gcn', 'trainer', (1, 1, 1, 1, 1, 1), graph=True),
    # ---- B: the other update rules at this size, trainer defaults (no fused Del-1; the weight-stationary GEMMs all the same)
    _c('B/gcn/both_all', 'gcn', 'trainer', (0, 0, 1, 1, 1, 1), loss_type='both_all'),
    _c('B/gcn/only1', 'gcn', 'trainer', (0, 0, 1, 0, 0, 1), loss_type='only1'),
    _c('B/gcn/only2_layerwise', 'gcn', 'trainer', (0, 0, 1, 0, 0, 1), loss_type='only2_layerwise'),
    _c('B/gcn/only2_all', 'gcn', 'trainer', (0, 0, 1, 0, 0, 1), loss_type='only2_all'),
    _c('B/gat/both_all', 'gat', 'trainer', (0, 0, 1, 1, 1, 1), loss_type='both_all'),
    _c('B/gat/only1', 'gat', 'trainer', (0, 0, 1, 0, 0, 1), loss_type='only1'),
    _c('B/gat/only2_layerwise', 'gat', 'trainer', (0, 0, 1, 0, 0, 1), loss_type='only2_layerwise'),
    _c('B/gat/only2_all', 'gat', 'trainer', (0, 0, 1, 0, 0, 1), loss_type='only2_all'),
    # ---- C: the KLD / cosine families (folded row-loss launches between the weight-stationary products)
    _c('C/gcn/kld_mean/plain', 'gcn', 'plain', (0, 0, 0, 1, 0, 1), loss_fct='kld_mean'),
    _c('C/gcn/kld_mean/trainer', 'gcn', 'trainer', (0, 0, 1, 1, 0, 1), loss_fct='kld_mean'),
    _c('C/gat/cosine_mean/trainer', 'gat', 'trainer', (0, 0, 1, 1, 0, 1), loss_fct='cosine_mean'),
    _c('C/gcn/cosine_sum/plain', 'gcn', 'plain', (0, 0, 0, 1, 0, 1), loss_fct='cosine_sum'),
    # ---- D: the knobs around the fused Del-1 step
    _c('D/gcn/plain/GD_NO_FUSED_L2', 'gcn', 'plain', (1, 1, 0, 1, 0, 1), knob='GD_NO_FUSED_L2'),
    _c('D/gcn/plain/GD_NO_FUSED_WGRAD2', 'gcn', 'plain', (1, 1, 0, 1, 0, 1), knob='GD_NO_FUSED_WGRAD2'),
    _c('D/gcn/plain/GD_DEL1_CHAIN=0', 'gcn', 'plain', (1, 0, 0, 1, 1, 1), knob=('GD_DEL1_CHAIN', '0')),
    _c('D/gcn/cache/GD_CACHE_SPLIT=0', 'gcn', 'cache', (0, 0, 0, 1, 1, 0), knob=('GD_CACHE_SPLIT', '0')),
    _c('D/gcn/plain/GD_NO_STEP_TAIL', 'gcn', 'plain', (0, 0, 0, 0, 0, 1), knob='GD_NO_STEP_TAIL'),
    _c('D/gcn/plain/GD_NO_FUSED_LOSS1', 'gcn', 'plain', (0, 0, 0, 1, 1, 1), knob='GD_NO_FUSED_LOSS1'),
    _c('D/gcn/plain/GD_NO_SPLIT', 'gcn', 'plain', (0, 0, 0, 1, 0, 0), knob='GD_NO_SPLIT'),
    _c('D/gat/plain/GD_DEL1_CHAIN=0', 'gat', 'plain', (1, 0, 0, 1, 1, 1), knob=('GD_DEL1_CHAIN', '0')),
    _c('D/gat/plain/GD_NO_GAT_RANK1_EPILOGUE', 'gat', 'plain', (1, 0, 0, 1, 1, 1), knob='GD_NO_GAT_RANK1_EPILOGUE'),
    _c('D/gat/plain/GD_NO_GAT_DOTS', 'gat', 'plain', (1, 1, 0, 1, 1, 1), knob='GD_NO_GAT_DOTS'),
    _c('D/sage/plain/GD_NO_FUSED_L2', 'sage', 'plain', (1, 0, 0, 1, 0, 1), knob='GD_NO_FUSED_L2'),
    _c('D/gcn/trainer/GD_DEL1_CHAIN=0', 'gcn', 'trainer', (1, 0, 1, 1, 1, 1), knob=('GD_DEL1_CHAIN', '0')),
    # ---- E: the fused-Del-1 forms plan_step can choose at this size that A - D leave out (test_engine_large_forms_cpu.py
    # enumerates them): each backbone with the layer-2 fusions off and, where it chains, unchained - on all rows and on the
    # affected rows
    _c('E/gcn/trainer/GD_NO_FUSED_L2', 'gcn', 'trainer', (1, 1, 1, 1, 0, 1), knob='GD_NO_FUSED_L2'),
    _c('E/gcn/trainer/GD_NO_FUSED_WGRAD2', 'gcn', 'trainer', (1, 1, 1, 1, 0, 1), knob='GD_NO_FUSED_WGRAD2'),
    _c('E/gin/plain/GD_NO_FUSED_L2', 'gin', 'plain', (1, 1, 0, 1, 0, 1), knob='GD_NO_FUSED_L2'),
    _c('E/gin/plain/GD_NO_FUSED_WGRAD2', 'gin', 'plain', (1, 1, 0, 1, 0, 1), knob='GD_NO_FUSED_WGRAD2'),
    _c('E/gin/plain/GD_DEL1_CHAIN=0', 'gin', 'plain', (1, 0, 0, 1, 1, 1), knob=('GD_DEL1_CHAIN', '0')),
    _c('E/gin/trainer/GD_NO_FUSED_L2', 'gin', 'trainer', (1, 1, 1, 1, 0, 1), knob='GD_NO_FUSED_L2'),
    _c('E/gin/trainer/GD_NO_FUSED_WGRAD2', 'gin', 'trainer', (1, 1, 1, 1, 0, 1), knob='GD_NO_FUSED_WGRAD2'),
    _c('E/gin/trainer/GD_DEL1_CHAIN=0', 'gin', 'trainer', (1, 0, 1, 1, 1, 1), knob=('GD_DEL1_CHAIN', '0')),
    _c('E/gat/plain/GD_NO_FUSED_L2', 'gat', 'plain', (1, 1, 0, 1, 0, 1), knob='GD_NO_FUSED_L2'),
    _c('E/gat/plain/GD_NO_FUSED_WGRAD2', 'gat', 'plain', (1, 1, 0, 1, 0, 1), knob='GD_NO_FUSED_WGRAD2'),
    _c('E/gat/trainer/GD_NO_FUSED_L2', 'gat', 'trainer', (1, 1, 1, 1, 0, 1), knob='GD_NO_FUSED_L2'),
    _c('E/gat/trainer/GD_NO_FUSED_WGRAD2', 'gat', 'trainer', (1, 1, 1, 1, 0, 1), knob='GD_NO_FUSED_WGRAD2'),
    _c('E/gat/trainer/GD_DEL1_CHAIN=0', 'gat', 'trainer', (1, 0, 1, 1, 1, 1), knob=('GD_DEL1_CHAIN', '0')),
    _c('E/gat/trainer/GD_NO_GAT_DOTS', 'gat', 'trainer', (1, 1, 1, 1, 1, 1), knob='GD_NO_GAT_DOTS'),
    _c('E/sage/plain/GD_NO_FUSED_WGRAD2', 'sage', 'plain', (1, 0, 0, 1, 0, 1), knob='GD_NO_FUSED_WGRAD2'),
    _c('E/sage/trainer/GD_NO_FUSED_L2', 'sage', 'trainer', (1, 0, 1, 1, 0, 1), knob='GD_NO_FUSED_L2'),
    _c('E/sage/trainer/GD_NO_FUSED_WGRAD2', 'sage', 'trainer', (1, 0, 1, 1, 0, 1), knob='GD_NO_FUSED_WGRAD2'),
]
BY_NAME = {c.name: c for c in CASES}


def knob_field(case):
    """(field of engine.Knobs, its value) of a case's environment variable, or None."""
    if case.knob is None:
        return None
    name, raw = case.knob
    return name[3:].lower(), raw != '0'


def plain_sibling(case):
    """The case of the same oracle key with no option and no knob - what a variant is compared with - or None."""
    for c in CASES:
        if ((c.gnn, c.loss_type, c.loss_fct) == (case.gnn, case.loss_type, case.loss_fct) and c.opts == 'plain' and c.knob is None
                and not c.graph and c is not case):
            return c
    return None


@functools.lru_cache(maxsize=None)
def large_request():
    """-> (data, neg, ni1, ni2): the request every test of this module and of test_engine_large_forms_cpu.py shares.  Built once
    per process on the host (about 2 s), never modified.  Negatives and NI masks as tests/dist_worker.py::small_request builds
    them."""
    from gnndelete_amd.framework.data import prepare_edge_deletion
    from gnndelete_amd.framework.graph_utils import negative_sampling
    from gnndelete_amd.framework.synth import make_linkpred_dataset
    from oracle import gnndelete_ref as R
    rng = torch.get_rng_state()
    data, dfm = make_linkpred_dataset(None, seed=SEED, shape=(N, F, M_EDGES, 'dense'))
    torch.manual_seed(SEED)
    prepare_edge_deletion(data, dfm['out'], N_DF)
    gen = torch.Generator().manual_seed(SEED)
    neg = negative_sampling(data.train_pos_edge_index, data.num_nodes, int(data.df_mask.sum()), generator=gen)
    ni1, ni2 = R.non_df_masks(data.num_nodes, data.directed_df_edge_index, data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
    torch.set_rng_state(rng)
    return data, neg, ni1, ni2


@functools.lru_cache(maxsize=None)
def _state(gnn):
    """The frozen backbone of a case, seeded, with Del weights away from the reference's ones / 1000 start (as the seeded
    requests of test_row_losses_engine_gpu.py): with that start every row of z1 and z2 is a multiple of the all-ones vector, so a
    Del product with a transposed or column-permuted weight is the same product, and Adam's first update (+-lr per entry) is as
    large as the weight itself - the cosine losses then follow a trajectory that correct fp32 arithmetic cannot hold (the fp32
    oracle ensemble ends 2e-2 ... 6e-2 from the fp64 oracle in W_D1 after six iterations of this request)."""
    from oracle import gnndelete_ref as R
    data = large_request()[0]
    rng = torch.get_rng_state()
    torch.manual_seed(SEED)
    mo = R.TwoLayerDelete(gnn, F, HID, OUT, data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        mo.deletion1.deletion_weight.copy_(torch.eye(HID) * 0.6 + 0.02 * torch.randn(HID, HID, generator=g))
        mo.deletion2.deletion_weight.copy_(torch.eye(OUT) * 0.7 + 0.05 * torch.randn(OUT, OUT, generator=g))
    torch.set_rng_state(rng)
    return {k: v.detach().clone() for k, v in mo.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _device_request():
    data, neg, ni1, ni2 = large_request()
    dev = torch.device('cuda')
    E = data.train_pos_edge_index.to(dev)
    return dict(x=data.x.to(dev), e_dr=E[:, data.dr_mask.to(dev)].contiguous(), e_sdf=E[:, data.sdf_mask.to(dev)].contiguous(),
                pos=E[:, data.df_mask.to(dev)].contiguous(), neg=neg.to(dev), m1=data.sdf_node_1hop_mask.to(dev),
                m2=data.sdf_node_2hop_mask.to(dev))


@functools.lru_cache(maxsize=None)
def _oracle(gnn, loss_type, loss_fct, iters=ITERS):
    """The oracle's run of a (gnn, loss_type, loss_fct) as torch ops on the device: the fp64 run - its train_loss log, Del
    weights, z1[S1] and z2[S2] on the retained edges - and the fp32 ensemble (edge lists as they are and permuted with seeds 1, 2):
    its Del weights and the distance of its embeddings to the fp64 run's.  Computed once, shared, never modified."""
    import gc
    from helpers import oracle_runner, rel_l2
    data, neg, ni1, ni2 = large_request()
    dev = torch.device('cuda')

    def run(dtype, perm):
        step, snap, _ = oracle_runner(gnn, data, _state(gnn), neg, ni1, ni2, dtype, dev, loss_type=loss_type, alpha=ALPHA, lr=LR,
                                      perm=perm, hidden=HID, out=OUT, loss_fct=loss_fct)
        logs = [step()['train_loss'] for _ in range(iters)]
        out = snap()[:4]
        del step, snap
        gc.collect()
        torch.cuda.empty_cache()
        return logs, out
    logs, (w1, w2, z1, z2) = run(torch.float64, None)
    ens_w, ens_z = [], []
    for perm in (None, 1, 2):
        _, (e1, e2, ez1, ez2) = run(torch.float32, perm)
        ens_w.append((e1, e2))
        ens_z.append((rel_l2(ez1, z1), rel_l2(ez2, z2)))
    return dict(logs=logs, w=(w1, w2), z=(z1.to(dev), z2.to(dev)), ens_w=ens_w, ens_z=ens_z)


def _run(case, monkeypatch=None):
    """The engine of a case on a fresh model: ITERS iterations, then what the assertions read (small host tensors and numbers)."""
    from gnndelete_amd import _lib
    from gnndelete_amd.engine import NodeembEngine, plan_step
    from helpers import hip_model, rel_l2
    data = large_request()[0]
    _, _, ni1, ni2 = large_request()
    d = _device_request()
    model = hip_model(case.gnn, _state(case.gnn), data.sdf_node_1hop_mask, data.sdf_node_2hop_mask)
    with torch.no_grad():
        z1o, z2o = model.get_original_embeddings(d['x'], d['e_dr'], return_all_emb=True)
    kw = dict(loss_type=case.loss_type, alpha=ALPHA, lr=LR, use_graph=case.graph, loss_fct=case.loss_fct, **OPTS[case.opts])
    if case.knob is not None:
        with monkeypatch.context() as mp:          # the engine reads its knobs in the constructor, once
            mp.setenv(*case.knob)
            eng = NodeembEngine(model, d['x'], d['e_sdf'], z1o, z2o, d['pos'], d['neg'], ni1, ni2, **kw)
    else:
        eng = NodeembEngine(model, d['x'], d['e_sdf'], z1o, z2o, d['pos'], d['neg'], ni1, ni2, **kw)
    for _ in range(ITERS):
        eng.step()
    hist = eng.loss_history()
    ref = _oracle(case.gnn, case.loss_type, case.loss_fct)
    with torch.no_grad():
        z1, z2 = model(d['x'], d['e_dr'], return_all_emb=True)
    dz = (rel_l2(z1[d['m1']].double(), ref['z'][0]), rel_l2(z2[d['m2']].double(), ref['z'][1]))
    return dict(forms=eng.forms, planned=plan_step(eng.facts, eng.knobs), knobs=eng.knobs, s1=eng.s1, s2=eng.s2, n=eng.n,
                ws_covers=bool(_lib.lib().gd_rows_gemm_ws_covers(eng.s1, HID, HID)), perm=eng.perm is not None,
                graph_replayed=eng._graph is not None, hist=hist,
                w=(model.deletion1.deletion_weight.detach().double().cpu(), model.deletion2.deletion_weight.detach().double().cpu()),
                w32=(model.deletion1.deletion_weight.detach().cpu().clone(), model.deletion2.deletion_weight.detach().cpu().clone()),
                dz=dz)


@functools.lru_cache(maxsize=None)
def _reference_run(name):
    """The run of a case without a knob, kept for the variants that are compared with it."""
    assert BY_NAME[name].knob is None
    return _run(BY_NAME[name])


def test_case_table_is_consistent():
    assert len(BY_NAME) == len(CASES)
    for c in CASES:
        assert c.opts in OPTS and set(c.flags) == set(FLAGS)
        assert c.knob is None or c.knob[0] not in ('GD_DEL1_FUSED', 'GD_ROWS_GEMM_WS', 'GD_DEL2_WS'), c.name


@pytest.mark.parametrize('name', [c.name for c in CASES])
def test_large_forms_match_the_fp64_oracle(name, monkeypatch):
    from gnndelete_amd.engine import Knobs
    from helpers import assert_del_weights_within_fp32_spread, rel_l2
    case = BY_NAME[name]
    got = _reference_run(name) if case.knob is None else _run(case, monkeypatch)
    ref = _oracle(case.gnn, case.loss_type, case.loss_fct)
    # ---- (a) the forms
    assert got['forms'] == got['planned']
    want_knobs = Knobs() if case.knob is None else Knobs()._replace(**dict([knob_field(case)]))
    assert got['knobs'] == want_knobs, 'the knob reached the constructor (and no other is set in this environment)'
    for flag, on in case.flags.items():
        assert getattr(got['forms'], flag) == on, (flag, got['forms'])
    assert WS_MIN_ROWS <= got['s1'] < got['s2'] < got['n'] and got['ws_covers'] and got['perm']
    assert got['graph_replayed'] == case.graph
    # ---- (b) the loss history
    hist = got['hist']
    assert hist.shape[0] == ITERS
    d_loss = max(abs(float(hist[i, 0]) - want) / abs(want) for i, want in enumerate(ref['logs']))
    d_ens = [max(rel_l2(e[k], ref['w'][k]) for e in ref['ens_w']) for k in (0, 1)]
    print(f'[{name}] MEASURED loss {d_loss:.1e} | z1[S1] {got["dz"][0]:.1e} (ens {max(e[0] for e in ref["ens_z"]):.1e}) | '
          f'z2[S2] {got["dz"][1]:.1e} (ens {max(e[1] for e in ref["ens_z"]):.1e}) | W_D1 {rel_l2(got["w"][0], ref["w"][0]):.1e} '
          f'(ens {d_ens[0]:.1e}) | W_D2 {rel_l2(got["w"][1], ref["w"][1]):.1e} (ens {d_ens[1]:.1e})')
    for i, want in enumerate(ref['logs']):
        assert abs(float(hist[i, 0]) - want) <= 1e-4 * abs(want), (i, float(hist[i, 0]), want)
    # ---- (c) the affected-node embeddings: 1e-4 as it stands wherever the fp32 ensemble is inside it
    for k, zname in enumerate(('z1[S1]', 'z2[S2]')):
        worst = max(e[k] for e in ref['ens_z'])
        if worst <= 1e-4:
            assert got['dz'][k] <= 1e-4, (zname, got['dz'][k], ref['ens_z'])
        else:
            print(f'[{name}] {zname}: the fp32 ENSEMBLE is {worst:.2e} from the fp64 oracle after {ITERS} iterations - outside 1e-4 on '
                  f'its own; HIP ({got["dz"][k]:.2e}) is held to twice that distance')
            assert got['dz'][k] <= 2.0 * worst, (zname, got['dz'][k], ref['ens_z'])
    # ---- (d) the Del weights
    assert_del_weights_within_fp32_spread(name, got['w'], ref['w'], ref['ens_w'], ITERS)
    # ---- (e) a variant against the plain engine of the same oracle key
    sib = plain_sibling(case)
    if sib is not None:
        base = _reference_run(sib.name)
        assert torch.allclose(hist[:, 0], base['hist'][:, 0], rtol=1e-5, atol=0), (hist[:, 0], base['hist'][:, 0])
        for a_, b_ in zip(got['w'], base['w']):
            assert rel_l2(a_, b_) < 2e-5, rel_l2(a_, b_)
    if case.graph:           # graph replay = the eager run of the same options, bit for bit
        eager = _reference_run(name[:-len('/graph')])
        assert torch.equal(hist, eager['hist'])
        assert torch.equal(got['w32'][0], eager['w32'][0]) and torch.equal(got['w32'][1], eager['w32'][1])


def test_the_bars_tell_update_rules_apart():
    """Teeth: the fp64 oracles of both_layerwise and both_all (GCN) differ only in the update rule - which gradient of the layer-2
    loss reaches W_D1, and when.  After ITERS iterations they must be further apart in W_D1 and in z1[S1] than ten times the
    bounds (c) and (d) hold the engine to, so that a step which drops or misroutes the layer-2 gradient cannot pass them."""
    from helpers import rel_l2
    a, b = _oracle('gcn', 'both_layerwise', 'mse_mean'), _oracle('gcn', 'both_all', 'mse_mean')
    sep_w, sep_z = rel_l2(a['w'][0], b['w'][0]), rel_l2(a['z'][0], b['z'][0])
    bound_w = max(max(2.0 * max(rel_l2(e[0], o['w'][0]) for e in o['ens_w']), 5e-5) for o in (a, b))
    bound_z = max(max(1e-4, 2.0 * max(e[0] for e in o['ens_z'])) for o in (a, b))
    print(f'[teeth] MEASURED both_layerwise vs both_all after {ITERS} iterations: W_D1 {sep_w:.2e} (bound {bound_w:.1e}), '
          f'z1[S1] {sep_z:.2e} (bound {bound_z:.1e})')
    assert sep_w > 10 * bound_w and sep_z > 10 * bound_z, (sep_w, bound_w, sep_z, bound_z)
