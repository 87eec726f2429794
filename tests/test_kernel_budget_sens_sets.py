"""Resources of the kernels of sens_sets.hip, read from the cross-compiled kernel descriptors (no GPU): no scratch, at
most 128 VGPRs, and the static LDS together with the most a launch adds within a workgroup's 64 KiB.

As built: sens_sets_kernel 52 VGPRs, and sens_sets_host.h's sens_sets_fold_kernel 22 and sens_sets_init_kernel 8; no
static LDS; the launch adds sens_sets_lds_doubles: 488 B at (Lmax, nper, nb) = (8, 5, 20), 3 216 B at (100, 60, 1024),
824 B at (20, 21, 200), and at its most -- few cells a period, so that a workgroup's 256 items touch every period --
50 080 B at (100, 60, 1)."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def test_sens_sets_kernels_use_no_scratch_and_fit_the_lds():
    from kernel_resources import kernel_resources
    from test_sens_sets import load_sim
    ssim = load_sim()
    r = kernel_resources('sens_sets.hip')
    main = {k: v for k, v in r.items() if 'sens_sets_kernel' in k}
    fold = {k: v for k, v in r.items() if 'sens_sets_fold_kernel' in k}
    assert len(main) == 1 and len(fold) == 1, sorted(r)
    for k, v in r.items():
        print('%-60s %3d VGPRs  %3d SGPRs  LDS %d B' % (k, v['vgpr'], v['sgpr'], v['lds']))
    assert all(v['scratch'] == 0 for v in r.values()), r
    assert all(v['vgpr'] <= 128 for v in r.values()), r                 # four waves per SIMD at least
    for Lmax, nper, nb in ((8, 5, 20), (100, 60, 1024), (20, 21, 200), (100, 60, 1), (100, 60, 3)):
        dyn = ssim.sss_lds_bytes(Lmax, nper, nb)
        # h, the tops, and c_out and G of every period 256 consecutive items can touch
        span = min(nper, 255 // (nb + 1) + 2)
        assert dyn == 8 * (2 * Lmax + span * (Lmax + 1)), (Lmax, nper, nb, dyn)
        for v in main.values():
            assert v['lds'] + dyn <= 64 * 1024, (Lmax, nper, nb, v, dyn)
    assert all(v['lds'] == 0 for v in fold.values())
    assert ssim.sss_threads() == 256 and ssim.sss_block_rows() == 256
