"""profiles/device_negatives.json from the records of one box: tools/experiments/backbone_fused.py of this tree (--backbone), the
same script of the PARENT commit run with the parent's library before and after it (--parent, two or more records),
tools/experiments/edgeprob_fused.py of this tree (--edgeprob).  `comparison` holds the synth-collab figures: the parent's fused
epoch and its run-to-run spread (max - min over all its regions), this tree's host-draw leg and device-draw leg, and whether a
speed-up may be stated - only when the device leg lies below the parent's epoch by more than the parent's own spread and
every device region lies below every parent region.

    python tools/experiments/device_negatives_record.py --backbone B.json --parent P1.json P2.json --edgeprob E.json \\
        [--out profiles/device_negatives.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from backbone_fused import parent_legs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--backbone', required=True)
    ap.add_argument('--parent', nargs='+', required=True)
    ap.add_argument('--edgeprob', default=None)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                                                  'profiles', 'device_negatives.json'))
    a = ap.parse_args()
    with open(a.backbone) as f:
        rec = json.load(f)
    parents = [p for p in parent_legs(a.parent) if p['graph'] == 'synth-collab' and p['request'] == 'original']
    collab = [r for r in rec['runs'] if r['graph'] == 'synth-collab' and r['request'] == 'original'][0]
    p_regions = [v for p in parents for v in p['fused_regions_ms']]
    p_medians = [p['fused_ms_per_epoch'] for p in parents]
    spread = round(max(p_regions) - min(p_regions), 4)
    parent_ms = round(sum(p_medians) / len(p_medians), 4)
    device_ms = collab['device_ms_per_epoch']
    comparison = {
        'graph': 'synth-collab', 'request': 'original', 'gnn': collab['gnn'],
        'parent_fused_ms_per_epoch_runs': p_medians, 'parent_fused_ms_per_epoch': parent_ms,
        'parent_regions_ms': p_regions, 'parent_run_to_run_spread_ms': spread,
        'parent_spread_is': 'max - min over all 30-epoch regions of the parent runs (before and after this tree\'s run, same box)',
        'host_leg_ms_per_epoch': collab['fused_ms_per_epoch'], 'host_leg_regions_ms': collab['fused_regions_ms'],
        'device_leg_ms_per_epoch': device_ms, 'device_leg_regions_ms': collab['device_regions_ms'],
        'device_below_parent_by_ms': round(parent_ms - device_ms, 4),
        'speed_up_may_be_stated': bool(parent_ms - device_ms > spread and max(collab['device_regions_ms']) < min(p_regions)),
        'parent_over_device': round(parent_ms / device_ms, 2),
    }
    full = {'kernel_source_stamp': rec['kernel_source_stamp'], 'comparison': comparison, 'runs': rec['runs'], 'parent': parents}
    if a.edgeprob:
        with open(a.edgeprob) as f:
            full['edgeprob_runs'] = json.load(f)['runs']
    with open(a.out, 'w') as f:
        json.dump(full, f, indent=1)
        f.write('\n')
    print(json.dumps(comparison))


if __name__ == '__main__':
    main()
