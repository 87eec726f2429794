"""Resources of ell_sens_root_kernel and ell_sens_kernel, checked on the cross-compiled gfx950 code object (no GPU):
exactly two kernels (Rayleigh only), no private (scratch) memory in either, and no static LDS (ell_sens_kernel's model
image is dynamic LDS, sized at the launch).  The VGPR counts are recorded in DESIGN.md section 4.1g, not asserted.
ell_sens_total.hip holds the one kernel of the layer total, without scratch or LDS."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))


def test_ell_sens_kernels_have_no_scratch():
    from kernel_resources import kernel_resources
    r = kernel_resources('ell_sens.hip')
    roots = sorted(n for n in r if n.startswith('ell_sens_root_kernel'))
    slots = sorted(n for n in r if n.startswith('ell_sens_kernel'))
    assert len(roots) == 1 and len(slots) == 1 and len(r) == 2, sorted(r)
    for name, row in r.items():
        assert row['scratch'] == 0 and row['lds'] == 0, (name, row)
        print(name, row)


def test_ell_sens_total_is_one_kernel_without_scratch():
    from kernel_resources import kernel_resources
    r = kernel_resources('ell_sens_total.hip')
    assert len(r) == 1 and list(r)[0].startswith('ell_sens_vs_total_kernel'), sorted(r)
    for name, row in r.items():
        assert row['scratch'] == 0 and row['lds'] == 0, (name, row)
        print(name, row)
