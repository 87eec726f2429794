// sens_pass.h -- what the three sensitivity passes share: phase velocity (sensitivity.hip), group velocity
// (sens_group.hip) and ellipticity (ell_sens.hip).  The argument blocks, the sizing of a launch, and the two lane bodies
// the six kernels are thin wrappers of.
//
// A pass is two kernels of SENS_PASS_T lanes per workgroup.
//
// The root kernel, one lane per (model, period): lane g is period g % nper of model g / nper.  It polishes the root the
// search stored -- straight-line FP64 work against 32 bytes of model per layer, so the layers are read where they lie --
// and writes c and what else its pass has per (model, period), NaN where there is no value.  sens_pass_root_lane is the
// decode and the question whether the row is a model at all; the pass supplies what is done with one as a callable.
//
// The slot kernel, one lane per (model, period, slot) with the slot the fastest index: lane g is slot g % (4 Lmax) of
// (model, period) g / (4 Lmax), so the 64 lanes of a wave hold the slots of one (model, period) -- of two at Lmax = 8,
// of at most 64 / (4 Lmax) + 2 -- and walk the layer recursion together: a perturbation moves a layer's value by 2^-14
// at most and with it no lane across a branch (trigonometric or hyperbolic per layer) the others do not take, except
// at a crossing.  Each lane evaluates one perturbed entry and writes one K.  The models a workgroup's lanes belong to
// (255 / (nper 4 Lmax) + 2 at most, 2 KiB / nper + 64 Lmax bytes, never the limit) are rounded to real*4 once and kept
// in dynamic LDS as doubles: a lane reads every layer 2 times per recursion, and the perturbed accessor (SensLay) is a
// compare and a select on the value read.  No scratch: no array is indexed at run time; no static LDS.
// sens_pass_slot_lane is all of it but the one value, which the pass supplies as a callable.
//
// The kernels are bound by their registers (DESIGN.md sections 4.1e-g have the counts), and four waves per workgroup
// put one on each SIMD whatever the number of workgroups a compute unit holds.
#pragma once
#include <hip/hip_runtime.h>
#include "sens_core.h"

namespace bh {

constexpr int SENS_PASS_T = 256;

struct SensPassArgs {
    int B, Lmax, nper;
    int mstride;             // elements between consecutive models in h/vp/vs/rho
    int c_stride, err_stride;
    const int *nlay;
    const double *h, *vp, *vs, *rho;
    const double *periods;   // [nper]
    const double *c;         // row b: c + b * c_stride, the phase velocities the search stored
    const int *c_err;        // row b: c_err[b * err_stride], the err flag of the target that wrote c
    double *K;               // [B][nper][4][Lmax]: the pass's own kernel, dc/dm, dU/dm or dE/dm
    double *c_out;           // [B][nper]
};

struct SensArgs : SensPassArgs {
    int iwave;               // 1 Love, 2 Rayleigh
    double *dc_dT;           // [B][nper]
    double *fc;              // [B][nper] workspace: F_c at the polished root
};

enum { SENS_GROUP_WS = 6 };  // doubles of workspace per (model, period)

struct SensGroupArgs : SensPassArgs {
    int iwave;               // 1 Love, 2 Rayleigh
    double *K_phase;         // K's shape: dc/dm at T, or null
    double *U, *dU_dT;       // [B][nper]
    double *ws;              // [SENS_GROUP_WS][B * nper] workspace: F_c, c+, F_c+, c-, F_c-, dc/dT
};

enum { ELL_SENS_WS = 3 };    // doubles of workspace per (model, period): F_c, G_c, sign(E) or 1

struct EllSensArgs : SensPassArgs {
    int absolute;            // != 0: E, dE/dT and K times sign(E)
    double *K_phase;         // K's shape: dc/dm, or null
    double *E, *dE_dT;       // [B][nper]
    double *ws;              // [ELL_SENS_WS][B * nper] workspace
};

hipError_t launch_sens(const SensArgs &A, hipStream_t stream);
hipError_t launch_sens_group(const SensGroupArgs &A, hipStream_t stream);
hipError_t launch_ell_sens(const EllSensArgs &A, hipStream_t stream);

inline long sens_pass_blocks(long lanes) { return (lanes + SENS_PASS_T - 1) / SENS_PASS_T; }

// B * nper * 4 * Lmax lanes must fit a grid: false when they do not (nothing is launched)
inline bool sens_pass_fits(const SensPassArgs &A)
{
    return sens_pass_blocks((long)A.B * A.nper * 4 * A.Lmax) <= 0x7fffffffL;
}

// the slot kernel's model image: the models a workgroup's lanes can belong to
inline size_t sens_pass_lds_bytes(const SensPassArgs &A)
{
    const long per_model = (long)A.nper * 4 * A.Lmax;
    return (size_t)((SENS_PASS_T - 1) / per_model + 2) * 4 * A.Lmax * sizeof(double);
}

// the two launches of a pass
template <class Args>
hipError_t sens_pass_launch(void (*root)(Args), void (*slot)(Args), const Args &A, hipStream_t stream)
{
    const long n1 = (long)A.B * A.nper, n2 = n1 * 4 * A.Lmax;
    hipLaunchKernelGGL(root, dim3((unsigned)sens_pass_blocks(n1)), dim3(SENS_PASS_T), 0, stream, A);
    hipLaunchKernelGGL(slot, dim3((unsigned)sens_pass_blocks(n2)), dim3(SENS_PASS_T), sens_pass_lds_bytes(A), stream, A);
    return hipGetLastError();
}

// A root kernel's lane g (the caller has checked g < B nper): model(b, k, nl, lay) for period k of model b with its nl
// layers `lay`, where the flag, the depth and the top layer say that row b is a model; not called where it is none.
template <class Model>
__device__ __forceinline__ void sens_pass_root_lane(const SensPassArgs &A, long g, Model model)
{
    const long b = g / A.nper;
    const int k = (int)(g - b * A.nper);
    const int nl = A.nlay[b];
    // the model is read only where the flag and the depth say that it is one (ell_kernel)
    if (A.c_err[b * A.err_stride] == 0 && nl >= 2 && nl <= A.Lmax) {
        const long m = b * A.mstride;
        const SensModelLay lay{A.h + m, A.vp + m, A.vs + m, A.rho + m};
        if (sens_model_ok(0, nl, A.Lmax, A.vs[m])) model(b, k, nl, lay);
    }
}

// A slot kernel's lane.  lds: the kernel's dynamic LDS (sens_pass_lds_bytes).  K_phase: null for a pass without one.
// value(lay, nl, k, pk, c, kind, idx, r0) -> the pass's K of slot (kind, idx) of layer image `lay` with nl layers at
// period k, (model, period) pk, polished root c; it may set r0, the phase kernel.
template <class Value>
__device__ __forceinline__ void sens_pass_slot_lane(const SensPassArgs &A, double *K_phase, double *lds, Value value)
{
    const int nslot = 4 * A.Lmax;
    const long per_model = (long)A.nper * nslot;
    const long total = (long)A.B * per_model;
    const long g0 = (long)blockIdx.x * SENS_PASS_T;
    const long b0 = g0 / per_model;
    long b1 = (g0 + SENS_PASS_T - 1) / per_model;
    if (b1 > A.B - 1) b1 = A.B - 1;
    // the block's models, [h | vp | vs | rho] of Lmax real*4 values each; 0 behind a model's last layer and for a row
    // that is no model of this batch
    const int nload = (int)(b1 - b0 + 1) * nslot;
    for (int j = threadIdx.x; j < nload; j += SENS_PASS_T) {
        const int m = j / nslot, s = j - m * nslot;
        const int kind = s / A.Lmax, i = s - kind * A.Lmax;
        const long b = b0 + m;
        const int nl = A.nlay[b];
        double v = 0.0;
        if (A.c_err[b * A.err_stride] == 0 && nl >= 2 && nl <= A.Lmax && i < nl) {
            const double *row = kind == SENS_H ? A.h : kind == SENS_VP ? A.vp : kind == SENS_VS ? A.vs : A.rho;
            v = (double)(float)row[b * A.mstride + i];
        }
        lds[j] = v;
    }
    __syncthreads();
    const long g = g0 + threadIdx.x;
    if (g >= total) return;
    const long pk = g / nslot;                       // (model, period)
    const int s = (int)(g - pk * nslot);
    const int kind = s / A.Lmax, idx = s - kind * A.Lmax;
    const long b = pk / A.nper;
    const int k = (int)(pk - b * A.nper);
    const double c = A.c_out[pk];
    double r, r0;
    if (c != c) {
        r = r0 = __builtin_nan("");                  // no value: the whole (model, period)
    } else {
        const int nl = A.nlay[b];                    // 2 .. Lmax: the root kernel wrote a c
        r = r0 = 0.0;                                // padding layers, the half-space's thickness
        if (idx < nl && !(kind == SENS_H && idx == nl - 1)) {
            const SensRows lay{lds + (b - b0) * nslot, A.Lmax};
            r = value(lay, nl, k, pk, c, kind, idx, r0);
        }
    }
    A.K[g] = r;
    if (K_phase) K_phase[g] = r0;
}

}  // namespace bh
