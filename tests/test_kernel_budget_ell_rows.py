"""Registers of ell_rows_kernel, checked on the cross-compiled kernel (no GPU): ell_kernel's straight-line FP64 code
with whole models per workgroup -- no scratch, the G-int flag array as its only LDS, and at most 128 VGPRs, so that the
four waves of a 256-thread workgroup fit the 512 registers of a SIMD lane.  (tests/test_kernel_budget_ell.py holds
ell_kernel and the dispersion and receiver-function kernels where they were.)"""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))

ELL_ROWS_VGPR = 104          # next_free_vgpr of ell_rows_kernel as this commit builds it (ell_kernel: 102)


def test_ell_rows_kernel_has_no_scratch_one_small_lds_array_and_its_pinned_registers():
    from kernel_resources import kernel_resources
    r = kernel_resources('ell_rows.hip')
    assert list(r) == ['ell_rows_kernel'], sorted(r)
    row = r['ell_rows_kernel']
    assert row['scratch'] == 0, row
    assert 0 < row['lds'] <= 1024, row
    assert row['vgpr'] <= 128 and row['vgpr'] == ELL_ROWS_VGPR, row
