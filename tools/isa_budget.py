"""Static instruction budget of a kernel: cross-compiles kernels.hip to gfx950 assembly (no GPU needed) and
prints, per basic block of the chosen kernel, the instruction counts by class -- fp64 VALU, other VALU, moves,
selects, LDS, SALU, waits.  Used for the per-phase budgets in DESIGN.md / profiles/r03_rf_instruction_budget.md
(dynamic totals come from the PMC pass, SQ_INSTS_VALU).

    python tools/isa_budget.py rf_kernelILb0 [min block size]      # mangled-name fragment
    python tools/isa_budget.py swd_kernel 8 --moves                # also: register moves (v_mov_b32 / v_mov_b64) per block

move_counts(frag) returns (vector instructions, register moves) of a kernel (tests/test_swd_state_moves.py).
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bayhunter_amd import _lib  # noqa: E402


def cls(op):
    if op.startswith('v_') and 'f64' in op:
        return 'v_f64'
    if op.startswith('v_mov') or op.startswith('v_accvgpr'):
        return 'v_mov'
    if op.startswith('v_cndmask'):
        return 'v_sel'
    if op.startswith('v_'):
        return 'v_other'
    if op.startswith('ds_'):
        return 'lds'
    if op.startswith(('global_', 'buffer_', 'scratch_', 'flat_')):
        return 'vmem'
    if op.startswith(('s_waitcnt', 's_nop')):
        return 's_wait'
    return 'salu' if op.startswith('s_') else 'other'


def is_move(op):
    """A plain register move: v_mov_b32 / v_mov_b64 in any encoding (the search state copied between register sets)."""
    return op.startswith(('v_mov_b32', 'v_mov_b64'))


def kernel_blocks(frag):
    """Basic blocks of the kernel whose mangled name holds `frag`: [{name, note, ins: [opcode, ...]}, ...]"""
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, 'k.s')
        flags = [f for f in _lib.HIPCC_FLAGS if f not in ('-shared', '-fPIC')]
        subprocess.run(['/opt/rocm/bin/hipcc'] + flags + ['--cuda-device-only', '-S', 'kernels.hip', '-o', asm],
                       cwd=_lib.CSRC, check=True, stderr=subprocess.DEVNULL)
        lines = open(asm).read().split('\n')
    start = next(i for i, l in enumerate(lines) if re.match(r'^_Z\w*%s\w*:' % re.escape(frag), l))
    end = next(i for i in range(start, len(lines)) if 's_endpgm' in lines[i])
    blocks, cur = [], dict(name='entry', note='', ins=[])
    blocks.append(cur)
    for l in lines[start + 1:end]:
        m = re.match(r'^(\.LBB\d+_\d+):\s*(;.*)?$', l)
        if m:
            cur = dict(name=m.group(1), note=(m.group(2) or '').strip('; '), ins=[])
            blocks.append(cur)
        elif l.startswith('\t') and not l.strip().startswith((';', '.')):
            cur['ins'].append(l.split()[0])
    return blocks


def move_counts(frag):
    ins = [o for b in kernel_blocks(frag) for o in b['ins']]
    return sum(o.startswith('v_') for o in ins), sum(is_move(o) for o in ins)


def main(frag, minsize=1, moves=False):
    blocks = kernel_blocks(frag)
    keys = ['v_f64', 'v_other', 'v_sel', 'v_mov', 'lds', 'vmem', 'salu', 's_wait']
    extra = ['valu', 'moves'] if moves else []
    print('%-12s %5s  %s  %s' % ('block', 'instr', '  '.join('%7s' % k for k in keys + extra), 'loop'))
    tot = collections.Counter()
    for b in blocks:
        c = collections.Counter(cls(o) for o in b['ins'])
        if moves:
            c['valu'] = sum(o.startswith('v_') for o in b['ins'])
            c['moves'] = sum(is_move(o) for o in b['ins'])
        tot.update(c)
        if len(b['ins']) >= minsize:
            print('%-12s %5d  %s  %s' % (b['name'], len(b['ins']), '  '.join('%7d' % c[k] for k in keys + extra), b['note'][:44]))
    print('%-12s %5d  %s' % ('total', sum(tot[k] for k in keys) + tot['other'], '  '.join('%7d' % tot[k] for k in keys + extra)))


if __name__ == '__main__':
    argv = [a for a in sys.argv[1:] if a != '--moves']
    main(argv[0], int(argv[1]) if len(argv) > 1 else 1, moves='--moves' in sys.argv)
