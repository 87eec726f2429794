"""Registers of ell_kernel, checked on the cross-compiled kernel (no GPU): straight-line FP64 code without LDS and
without scratch, at the VGPR count its gfx950 build reports -- and adding it (ell_core.h includes swd_core.h, which it
does not change) must not have cost the dispersion and receiver-function kernels a register."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))

ELL_VGPR = 102          # next_free_vgpr of ell_kernel as this commit builds it
# next_free_vgpr read at commit 0dda5d1 (the parent of the ellipticity)
PARENT_VGPR = {'swd_kernel': 189, 'swd_team_kernel': 125, 'swd_team128_kernel': 146, 'swd_team256_kernel': 146,
               'swd_team512_kernel': 146, 'swd_team32_kernel': 193, 'swd_team16_kernel': 197, 'swd_team8_kernel': 195,
               'rf_kernel<false>': 128, 'rf_kernel<true>': 128, 'rf_kernel<false, true>': 128}


def test_ell_kernel_has_no_scratch_no_lds_and_its_pinned_registers():
    from kernel_resources import kernel_resources
    r = kernel_resources('ellipticity.hip')
    assert list(r) == ['ell_kernel'], sorted(r)
    row = r['ell_kernel']
    assert row['scratch'] == 0 and row['lds'] == 0, row
    assert row['vgpr'] == ELL_VGPR, row


def test_the_other_kernels_did_not_move():
    from kernel_resources import kernel_resources
    r = kernel_resources()
    for name, vgpr in PARENT_VGPR.items():
        assert r[name]['vgpr'] == vgpr and r[name]['scratch'] == 0, (name, r[name])
