"""Resources of the kernels of interfaces.hip, read from the cross-compiled kernel descriptors (no GPU): no scratch,
and the static LDS together with the most a launch adds within a workgroup's 64 KiB.

As built: interfaces_count_kernel 40 VGPRs (float32 and float64 rows), interfaces_moment_kernel 26 (float32) and 28
(float64); 16 B of static LDS in the count kernel (its two weight counters), none in the moment kernel."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def test_interfaces_kernels_use_no_scratch_and_fit_the_lds():
    from kernel_resources import kernel_resources
    from bayhunter_amd import _lib
    from test_interfaces import load_sim
    isim = load_sim()
    r = kernel_resources('interfaces.hip')
    count = {k: v for k, v in r.items() if 'interfaces_count_kernel' in k}
    moment = {k: v for k, v in r.items() if 'interfaces_moment_kernel' in k}
    assert len(count) == 2 and len(moment) == 2, sorted(r)              # float32 and float64 rows
    assert all(v['scratch'] == 0 for v in r.values()), r
    for k, v in r.items():
        print('%-60s %3d VGPRs  %3d SGPRs  LDS %d B' % (k, v['vgpr'], v['sgpr'], v['lds']))
    # dynamic LDS at its most: the cells of one group of depth bins; four waves' accumulators of every depth bin
    most_d, most_j = _lib.INTERFACES_MAX_DEPTH_BINS, _lib.INTERFACES_MAX_JUMP_BINS
    for nbd, nbj in ((20, 8), (400, 64), (most_d, most_j), (most_d, 0), (1, most_j)):
        group = isim.ifs_group(nbd, nbj)
        assert 1 <= group <= nbd
        for v in count.values():
            assert v['lds'] <= 64 * 1024 and v['lds'] + 8 * group * (6 + nbj) <= 64 * 1024, (nbd, nbj, group, v)
        for v in moment.values():
            assert v['lds'] <= 64 * 1024 and v['lds'] + 8 * 4 * nbd <= 64 * 1024, (nbd, v)
    assert isim.ifs_group(20, 8) == 20 and isim.ifs_group(400, 64) < 400        # the two paths of the GPU tier
    for v in list(count.values()) + list(moment.values()):
        assert v['vgpr'] <= 128, v                                       # four waves per SIMD at least
