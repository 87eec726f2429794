"""Register budget of the per-row form of rf_kernel (every model at the ray parameter of its own set), checked on the
cross-compiled kernels (no GPU): it has to fit beside swd_kernel exactly like the uniform form (2 x 192 + 128 VGPRs
per SIMD, tests/test_kernel_budget.py), and adding it must not have cost the existing kernels a register."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))

# next_free_vgpr read at commit dcdf91a (the parent of the per-row form)
PARENT_VGPR = {'rf_kernel<false>': 128, 'rf_kernel<true>': 128, 'swd_kernel': 189}


def _alloc(n):
    return -(-n // 8) * 8          # VGPRs are allocated in blocks of 8


def test_per_row_rf_kernel_fits_beside_swd_kernel_and_the_others_did_not_move():
    from kernel_resources import kernel_resources
    r = kernel_resources()
    assert 'rf_kernel<false, true>' in r, sorted(r)
    row = r['rf_kernel<false, true>']
    assert row['scratch'] == 0 and _alloc(row['vgpr']) <= 128, row
    assert 2 * _alloc(r['swd_kernel']['vgpr']) + _alloc(row['vgpr']) <= 512
    for name, vgpr in PARENT_VGPR.items():
        assert r[name]['vgpr'] == vgpr and r[name]['scratch'] == 0, (name, r[name])
