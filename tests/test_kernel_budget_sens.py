"""Resources of sens_root_kernel and sens_kernel, checked on the cross-compiled gfx950 code object (no GPU): no private
(scratch) memory in either, for either wave type, and no static LDS (sens_kernel's model image is dynamic LDS, sized
at the launch).  The VGPR counts are recorded in DESIGN.md section 4.1e, not asserted."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))


def test_sens_kernels_have_no_scratch():
    from kernel_resources import kernel_resources
    r = kernel_resources('sensitivity.hip')
    roots = sorted(n for n in r if n.startswith('sens_root_kernel'))
    slots = sorted(n for n in r if n.startswith('sens_kernel'))
    assert len(roots) == 2 and len(slots) == 2 and len(r) == 4, sorted(r)          # Love and Rayleigh of each
    for name, row in r.items():
        assert row['scratch'] == 0 and row['lds'] == 0, (name, row)
        print(name, row)
