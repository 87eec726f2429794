"""Resources of sens_group_root_kernel and sens_group_kernel, checked on the cross-compiled gfx950 code object (no GPU):
exactly four kernels (Love and Rayleigh of each), no private (scratch) memory in any, and no static LDS
(sens_group_kernel's model image is dynamic LDS, sized at the launch).  The VGPR counts are recorded in DESIGN.md
section 4.1f, not asserted."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))


def test_sens_group_kernels_have_no_scratch():
    from kernel_resources import kernel_resources
    r = kernel_resources('sens_group.hip')
    roots = sorted(n for n in r if n.startswith('sens_group_root_kernel'))
    slots = sorted(n for n in r if n.startswith('sens_group_kernel'))
    assert len(roots) == 2 and len(slots) == 2 and len(r) == 4, sorted(r)
    for name, row in r.items():
        assert row['scratch'] == 0 and row['lds'] == 0, (name, row)
        print(name, row)
