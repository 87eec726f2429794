"""Resources of rf_sens_kernel, checked on the cross-compiled gfx950 code object (no GPU): exactly two kernels (the
paired and the sequential form), no private (scratch) memory in either -- the sequential form's kept trace stays in
registers -- and no static LDS (the variants' blocks are dynamic LDS, sized at the launch).  The paired form fits the
four waves per SIMD its LDS budget is sized for (at most 128 VGPRs).  The VGPR counts are recorded in DESIGN.md section
4.1h."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))


def test_rf_sens_kernels_have_no_scratch():
    from kernel_resources import kernel_resources
    r = kernel_resources('rf_sens.hip')
    assert sorted(r) == ['rf_sens_kernel<false>', 'rf_sens_kernel<true>'], sorted(r)
    for name, row in r.items():
        assert row['scratch'] == 0 and row['lds'] == 0, (name, row)
        print(name, row)
    assert r['rf_sens_kernel<true>']['vgpr'] <= 128
