"""NodeembEngine with layer 1's aggregation on the wide 128-float form (gd_spmm_csr_onepass_wide128_f32), on the 80,001-node request
of test_explicit_chain_engine_gpu.py (the GCN step folded in layer 1), six iterations: the aggregation reaches the new entry, both Del weights stay inside that
test's bound to the fp64 oracle (1e-4 rel-L2, 1e-4 on every train_loss), and GD_SPMM_D128_FORM=items sends every 128-float
aggregation back to gd_spmm_csr_onepass_f32 - the launch of the step before this form - with the bits of a run whose routing never
knew the wide form."""
import functools

import pytest
import torch

from test_engine_large_forms_gpu import ITERS
from test_explicit_chain_engine_gpu import _engine
from test_layer1_fold_engine_gpu import _oracle64

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _six_steps(form):
    """form: None (the default routing), 'items' (the switch), 'never' (ops.spmm_wide128_form replaced by a constant False)."""
    from gnndelete_amd import _lib, ops
    calls = {'wide128': 0, 'items128': 0}
    with pytest.MonkeyPatch.context() as mp:
        if form == 'items':
            mp.setenv('GD_SPMM_D128_FORM', 'items')
        else:
            mp.delenv('GD_SPMM_D128_FORM', raising=False)
        if form == 'never':
            mp.setattr(ops, 'spmm_wide128_form', lambda *a, **k: False)
        handle = _lib.lib()
        wide, item = handle.gd_spmm_csr_onepass_wide128_f32, handle.gd_spmm_csr_onepass_f32

        def wide_probe(*a):
            calls['wide128'] += 1
            return wide(*a)

        def item_probe(*a):
            calls['items128'] += int(a[11] == 128)
            return item(*a)
        mp.setattr(handle, 'gd_spmm_csr_onepass_wide128_f32', wide_probe, raising=False)
        mp.setattr(handle, 'gd_spmm_csr_onepass_f32', item_probe, raising=False)
        eng, model = _engine(True)
        for _ in range(ITERS):
            eng.step()
        torch.cuda.synchronize()
    return dict(hist=eng.loss_history(), calls=calls,
                w=(model.deletion1.deletion_weight.detach().cpu().clone(), model.deletion2.deletion_weight.detach().cpu().clone()))


def test_wide128_step_against_the_fp64_oracle():
    from helpers import rel_l2
    got = _six_steps(None)
    assert got['calls']['wide128'] >= ITERS
    logs, w1, w2 = _oracle64()
    d_loss = max(abs(float(got['hist'][i, 0]) - want) / abs(want) for i, want in enumerate(logs))
    e1, e2 = rel_l2(got['w'][0].double(), w1), rel_l2(got['w'][1].double(), w2)
    print(f'[wide128 engine] MEASURED to the fp64 oracle after {ITERS} iterations: loss {d_loss:.1e}, W_D1 {e1:.1e}, W_D2 {e2:.1e}')
    assert got['hist'].shape[0] == ITERS
    assert d_loss <= 1e-4 and e1 < 1e-4 and e2 < 1e-4


def test_items_switch_restores_the_item_kernel_and_its_bits():
    a, b = _six_steps('items'), _six_steps('never')
    assert a['calls']['wide128'] == 0 and a['calls']['items128'] >= ITERS and b['calls'] == a['calls']
    assert torch.equal(a['hist'], b['hist']) and all(torch.equal(x, y) for x, y in zip(a['w'], b['w']))
    wide = _six_steps(None)
    # the same aggregations, on the other entry (the backbone's own forward passes keep the item kernel in both runs)
    assert wide['calls']['wide128'] == a['calls']['items128'] - wide['calls']['items128']
