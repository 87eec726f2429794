"""Resources of the kernels of rf_sens_sets.hip, read from the cross-compiled kernel descriptors (no GPU): no scratch, at
most 128 VGPRs, and the static LDS together with the most a launch adds within a workgroup's 64 KiB.

As built: rf_sens_sets_kernel 89 VGPRs with four samples a thread (with eight it took 166, and spilled under the bound of
128), and sens_sets_host.h's sens_sets_fold_kernel 22 and sens_sets_init_kernel 8; no static LDS; the launch adds h, the
tops, G[Lmax][16] and the tile's 16 sample offsets: 1 216 B at Lmax = 8, 14 464 B at Lmax = 100, whatever the samples and
the bins."""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def test_rf_sens_sets_kernels_use_no_scratch_and_fit_the_lds():
    from bayhunter_amd import _lib
    from kernel_resources import kernel_resources
    from test_rf_sens_sets import load_sim
    rsim = load_sim()
    r = kernel_resources('rf_sens_sets.hip')
    main = {k: v for k, v in r.items() if 'rf_sens_sets_kernel' in k}
    fold = {k: v for k, v in r.items() if 'sens_sets_fold_kernel' in k}
    assert len(main) == 1 and len(fold) == 1, sorted(r)
    for k, v in r.items():
        print('%-60s %3d VGPRs  %3d SGPRs  LDS %d B' % (k, v['vgpr'], v['sgpr'], v['lds']))
    assert all(v['scratch'] == 0 for v in r.values()), r
    assert all(v['vgpr'] <= 128 for v in r.values()), r                 # four waves per SIMD at least
    rs, ts = rsim.rss_rs(), rsim.rss_tile_samples()
    assert rsim.rss_threads() == 256 and rsim.rss_tile_cells() * ts == 256 * rs
    for Lmax in (1, 8, 20, _lib.MAX_LAYERS):                            # the test shapes and the limit
        dyn = rsim.rss_lds_bytes(Lmax)
        assert dyn == 8 * (2 + ts) * Lmax + 4 * ts, (Lmax, dyn)
        for v in main.values():
            assert v['lds'] + dyn <= 64 * 1024, (Lmax, v, dyn)
    assert all(v['lds'] == 0 for v in fold.values())
