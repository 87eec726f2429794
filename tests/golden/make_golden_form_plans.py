"""What the form planner answers over a grid of calls (bh_swd_plan_forms, host only: no GPU), and which widths
bh_swd_set_forms takes -- recorded from the built library, so that a change to swd_launch.hip that is meant to leave the
plans alone can be held to it (tests/test_capi_host.py: test_form_plans_are_the_recorded_ones).

    python tests/golden/make_golden_form_plans.py      (writes tests/golden/form_plans.json)

form_plans.json was written by the library of commit 6e524ec, the parent of the commit that added this file.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'form_plans.json')

BATCHES = [1, 64, 512, 2048, 3000, 4096, 8192, 12288, 16384, 65536, 524288]
DEPTHS = [2, 3, 5, 6, 7, 10, 12, 14, 20, 21, 31, 60]
CUS = [256, 64]
# (iwave, igr, nper) per target
TARGET_SETS = {
    'rayleigh_phase_21': [(2, 0, 21)],
    'cfg3': [(2, 0, 40), (2, 1, 40), (1, 0, 40), (1, 1, 40)],
    'rayleigh_group_40_love_phase_21': [(2, 1, 40), (1, 0, 21)],
}
# bh_swd_hint before the call: none, (mean layers, calls in flight); 'half': mean layers = Lmax / 2
HINTS = [None, (4.8, 1), (4.8, 2), ('half', 4)]
MODE_SHAPE = (4096, 10, 'cfg3')                     # every bh_swd_set_kernel mode at this one shape
SET_FORMS_WIDTHS = [-8, -1, 0, 1, 2, 4, 7, 8, 9, 12, 16, 24, 32, 33, 48, 63, 64, 65, 96, 128, 192, 256, 384, 512, 1024]


def record(lib):
    """The planner's answers as a dictionary of lists (what form_plans.json holds)."""
    from bayhunter_amd import _lib

    def plan(B, L, specs, cus, hint=None):
        tg = (_lib.SwdTarget * len(specs))()
        off = 0
        for i, (iwave, igr, nper) in enumerate(specs):
            tg[i] = _lib.SwdTarget(iwave, igr, 1, 0, nper, off, off, 0)
            off += nper
        if hint is not None:
            _lib.check(lib.bh_swd_hint(L / 2.0 if hint[0] == 'half' else hint[0], hint[1]))
        forms = (C.c_int * len(specs))()
        _lib.check(lib.bh_swd_plan_forms(B, L, len(specs), tg, cus, forms))
        return list(forms)

    _lib.check(lib.bh_swd_set_kernel(0))
    _lib.check(lib.bh_swd_set_forms(None, 0))
    rec = {'plans': {}, 'modes': {}, 'set_forms': {}}
    for cus in CUS:
        for name in sorted(TARGET_SETS):
            for ih, hint in enumerate(HINTS):
                for B in BATCHES:
                    rec['plans']['cus %d | %s | hint %d | B %d' % (cus, name, ih, B)] = [
                        plan(B, L, TARGET_SETS[name], cus, hint) for L in DEPTHS]
    try:
        for mode in range(0, 9):
            _lib.check(lib.bh_swd_set_kernel(mode))
            rec['modes']['%d' % mode] = plan(MODE_SHAPE[0], MODE_SHAPE[1], TARGET_SETS[MODE_SHAPE[2]], 256)
    finally:
        lib.bh_swd_set_kernel(0)
    rec['modes']['-1'] = [lib.bh_swd_set_kernel(-1), lib.bh_last_error().decode()]
    rec['modes']['9'] = [lib.bh_swd_set_kernel(9), lib.bh_last_error().decode()]
    # bh_swd_set_forms: return code, and the error text of a refusal; an accepted width is what the planner then answers
    try:
        for w in SET_FORMS_WIDTHS:
            rc = lib.bh_swd_set_forms((C.c_int * 2)(0, w), 2)
            rec['set_forms']['%d' % w] = [rc, plan(64, 10, [(2, 0, 21), (1, 0, 21)], 256) if rc == 0
                                          else lib.bh_last_error().decode()]
        for key, forms in (('four forms', [0, 8, 16, 32]), ('seventeen targets', [64] * 17), ('three forms', [0, 8, 8, 512])):
            rc = lib.bh_swd_set_forms((C.c_int * len(forms))(*forms), len(forms))
            rec['set_forms'][key] = [rc, '' if rc == 0 else lib.bh_last_error().decode()]
    finally:
        lib.bh_swd_set_forms(None, 0)
    return rec


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    import bayhunter_amd
    bayhunter_amd.build()
    rec = record(bayhunter_amd.load())
    with open(OUT, 'w') as fh:
        fh.write('{\n')
        for i, sec in enumerate(sorted(rec)):
            fh.write(' %s: {\n' % json.dumps(sec))
            keys = list(rec[sec])
            fh.write(',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(rec[sec][k], separators=(',', ':'))) for k in keys))
            fh.write('\n }%s\n' % (',' if i + 1 < len(rec) else ''))
        fh.write('}\n')
    print('%s: %d bytes' % (OUT, os.path.getsize(OUT)))
