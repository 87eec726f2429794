// math_probe.h -- the fp64 primitives of bh_math.h, bh_common.h, rf_core.h and swd_team.h, one call each.
//
// Every number the library produces goes through these functions, and each has two sides: what hipcc compiles for the
// device and what g++ compiles under BH_HOSTSIM for the host replay (the other side of every #if).  math_probe_apply
// applies primitive `op` to one element -- up to MP_IN input doubles, up to MP_OUT output doubles, unused outputs 0 --
// and is compiled for both: by math_probe.hip into a kernel of its own (bh_selftest_math, include/bayhunter_amd.h) and
// by tests/hostsim/math_probe_sim.cpp with the flags of the device-math replay.  tests/test_math_probe.py (host) and
// tests/test_gpu_math_probe.py (device against host bit for bit, and against extended precision) drive them.
// The headers are included as kernels.hip includes them, so the primitives are the library's own, under its flags.
//
// The kernel's contract, which the rf_cexp_pair tests rely on: workgroups of 256 threads, thread i handles element i
// behind an `i < n` guard.  Wave w therefore holds elements 64 w .. 64 w + 63, in lane order, and the last wave is
// partly inactive when n is no multiple of 64.
//
// xdiv, xsqrt, xsqrt_recip_nz and recip_sq are not here: bh_selftest_division compares them on the device.
#pragma once
#include "bh_common.h"
#include "bh_math.h"
#include "rf_core.h"
#include "swd_core.h"
#include "swd_team.h"

namespace bh {

enum { MP_IN = 6, MP_OUT = 4 };
enum MathProbeOp {            // inputs                         -> outputs
    MP_SINCOS = 0,            // x                              -> sin, cos           bh_sincos
    MP_EXP,                   // x                              -> exp                bh_exp
    MP_EXP_BOUNDED,           // x                              -> exp                bh_exp_bounded
    MP_EXP_SMALL,             // x                              -> exp                rf_exp_small
    MP_CEXP,                  // re, im                         -> re, im             cexp_
    MP_CEXP_BOUNDED,          // re, im                         -> re, im             cexp_bounded
    MP_CEXP_PAIR,             // za.re, za.im, zb.re, zb.im     -> ea.re, ea.im, eb.re, eb.im   rf_cexp_pair
    MP_FRCP,                  // x                              -> 1/x                frcp
    MP_FSQRT,                 // x                              -> root               fsqrt
    MP_FSQRT_HINV,            // x                              -> g, h               fsqrt_hinv
    MP_CRECIP,                // re, im                         -> re, im             crecip
    MP_CSQRT_FAST,            // re, im                         -> re, im             csqrt_fast
    MP_CSQRT,                 // re, im                         -> re, im             csqrt_
    MP_CDIV,                  // x.re, x.im, y.re, y.im         -> re, im             operator/(cd, cd)
    MP_CMUL,                  // a.re, a.im, b.re, b.im         -> re, im             cmul(cd, cd)
    MP_CMADD,                 // acc.re, acc.im, a.., b..       -> re, im             cmadd(cd, cd, cd)
    MP_CMSUB,                 // acc.re, acc.im, a.., b..       -> re, im             cmsub(cd, cd, cd)
    MP_NEGATE_IF2,            // x, two (0 or 2)                -> x or -x            bh_negate_if2
    MP_SIGNS_DIFFER,          // a, b                           -> 0 or 1             bh_signs_differ
    MP_SCAN_CELL,             // base, cell (0 .. 63)           -> b, cn              swd_scan_cell
    MP_NOPS
};

BH_DEV void math_probe_apply(int op, const double *in, double *out)
{
    out[0] = out[1] = out[2] = out[3] = 0.0;
    cd z, w;
    switch (op) {
    case MP_SINCOS: bh_sincos(in[0], &out[0], &out[1]); break;
    case MP_EXP: out[0] = bh_exp(in[0]); break;
    case MP_EXP_BOUNDED: out[0] = bh_exp_bounded(in[0]); break;
    case MP_EXP_SMALL: out[0] = rf_exp_small(in[0]); break;
    case MP_CEXP: z = cexp_(mk(in[0], in[1])); out[0] = z.re; out[1] = z.im; break;
    case MP_CEXP_BOUNDED: z = cexp_bounded(mk(in[0], in[1])); out[0] = z.re; out[1] = z.im; break;
    case MP_CEXP_PAIR:
        rf_cexp_pair(mk(in[0], in[1]), mk(in[2], in[3]), &z, &w);
        out[0] = z.re; out[1] = z.im; out[2] = w.re; out[3] = w.im;
        break;
    case MP_FRCP: out[0] = frcp(in[0]); break;
    case MP_FSQRT: out[0] = fsqrt(in[0]); break;
    case MP_FSQRT_HINV: fsqrt_hinv(in[0], &out[0], &out[1]); break;
    case MP_CRECIP: z = crecip(mk(in[0], in[1])); out[0] = z.re; out[1] = z.im; break;
    case MP_CSQRT_FAST: z = csqrt_fast(mk(in[0], in[1])); out[0] = z.re; out[1] = z.im; break;
    case MP_CSQRT: z = csqrt_(mk(in[0], in[1])); out[0] = z.re; out[1] = z.im; break;
    case MP_CDIV: z = mk(in[0], in[1]) / mk(in[2], in[3]); out[0] = z.re; out[1] = z.im; break;
    case MP_CMUL: z = cmul(mk(in[0], in[1]), mk(in[2], in[3])); out[0] = z.re; out[1] = z.im; break;
    case MP_CMADD:
        z = cmadd(mk(in[0], in[1]), mk(in[2], in[3]), mk(in[4], in[5]));
        out[0] = z.re; out[1] = z.im;
        break;
    case MP_CMSUB:
        z = cmsub(mk(in[0], in[1]), mk(in[2], in[3]), mk(in[4], in[5]));
        out[0] = z.re; out[1] = z.im;
        break;
    case MP_NEGATE_IF2: out[0] = bh_negate_if2(in[0], in[1] != 0.0 ? 2 : 0); break;
    case MP_SIGNS_DIFFER: out[0] = bh_signs_differ(in[0], in[1]) ? 1.0 : 0.0; break;
    case MP_SCAN_CELL: swd_scan_cell(in[0], (int)in[1], &out[0], &out[1]); break;
    default: break;
    }
}

#if !defined(BH_HOSTSIM)
// n elements of primitive `op`: in [n][MP_IN], out [n][MP_OUT], device pointers (math_probe.hip)
hipError_t launch_math_probe(int op, long n, const double *in, double *out, hipStream_t stream);
#endif

}  // namespace bh
