"""Registers of datacov_kernel, checked on the cross-compiled kernel (no GPU): no scratch and no register spilled to
memory, a unified register file that leaves room for two waves per SIMD (a workgroup's eight waves on the four SIMDs of
one CU), the static LDS beside the stages within a CU's 160 KB, and the FP64 matrix instruction in the listing -- 48 per
kernel: 12 tile pairs a wave, four k-steps a stage."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


@pytest.fixture(scope='module')
def listing():
    from bayhunter_amd import _lib
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, 'datacov.s')
        flags = [f for f in _lib.HIPCC_FLAGS if f not in ('-shared', '-fPIC')]
        subprocess.run(['/opt/rocm/bin/hipcc'] + flags + ['--cuda-device-only', '-S', 'datacov.hip', '-o', asm],
                       cwd=_lib.CSRC, check=True, stderr=subprocess.DEVNULL)
        return open(asm).read()


def test_datacov_kernels_have_no_scratch_and_two_waves_per_simd():
    from kernel_resources import kernel_resources
    from test_datacov import load_sim
    r = kernel_resources('datacov.hip')
    mine = {k: v for k, v in r.items() if 'datacov_kernel' in k}
    assert len(mine) == 2, sorted(r)                                   # float32 and float64 rows
    assert sum('datacov_weight_kernel' in k for k in r) == 2 and any('datacov_fold_kernel' in k for k in r)
    assert any('datacov_unpack_kernel' in k for k in r)
    assert all(v['scratch'] == 0 for v in r.values()), r
    dsim = load_sim()
    for k, v in mine.items():
        # static: the block's two weight counters and the stage rows' weights; dynamic: the stages (datacov_core.h)
        assert v['lds'] == 16 + 2 * 16 * 4, (k, v)
        assert v['lds'] + dsim.dcs_max_lds_bytes() <= 160 * 1024, (k, v)
        # next_free_vgpr counts the unified file, accumulation registers included: 512 per SIMD lane, so two waves of a
        # workgroup's eight per SIMD at 256 or fewer.  (As built: 162 -- 12 accumulators of 8 registers, the operands,
        # the tile offsets, addresses, and the lanes that hold the scalar registers the compiler parks in a VGPR.)
        assert v['vgpr'] <= 256, (k, v)


def test_nothing_spills_to_memory_and_the_matrix_instruction_is_there(listing):
    kernels = re.findall(r'\.name:\s+(\S*datacov\S*)\n(.*?)\.wavefront_size', listing, re.S)
    assert len(kernels) == 6, [k for k, _ in kernels]
    for name, meta in kernels:
        assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', meta).group(1)) == 0, name
    bodies = re.findall(r'^(_ZN\S*datacov_kernel\S*):[^\n]*\n(.*?)\n\s*s_endpgm', listing, re.S | re.M)
    assert len(bodies) == 2, [n for n, _ in bodies]
    for name, body in bodies:
        assert body.count('v_mfma_f64_16x16x4_f64') == 48, (name, body.count('v_mfma_f64_16x16x4_f64'))
