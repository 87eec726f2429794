"""Register moves in swd_kernel, counted on the cross-compiled kernel (no GPU).

The throughput kernel is bound by vector issue, and a v_mov_b64 takes an issue slot like a v_fma_f64.  Written as
nested divergent arms, the control code (swd_control, swd_neville) and the driver's loop made the compiler keep
an old and a new copy of the Neville table and of much of the search state across every join: 856 of the
kernel's 3 056 vector instructions were v_mov_b32 / v_mov_b64 (parent 3ea2124).  With the state written once,
by selects at the top level, and the events taken in one straight-line pass the kernel
has 366 moves among 2 560 vector instructions.

Ceiling: 366 + 10 % for compiler noise = 402, which lies under half of the parent's 856 (428).  The narrow team
kernels (swd_team8 / 16 / 32) were not touched and are not counted here.
"""
import os
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))

PARENT_MOVES = 856
BRANCH_MOVES = 366
CEILING = BRANCH_MOVES + BRANCH_MOVES // 10          # 402


def test_ceiling_is_under_half_of_the_parent():
    assert CEILING < PARENT_MOVES / 2


def test_swd_kernel_register_moves():
    from isa_budget import move_counts
    valu, moves = move_counts('swd_kernel')
    print('swd_kernel: %d vector instructions, %d register moves (ceiling %d)' % (valu, moves, CEILING))
    assert valu > 1000, valu                          # the kernel was found and parsed
    assert moves <= CEILING, (valu, moves)
