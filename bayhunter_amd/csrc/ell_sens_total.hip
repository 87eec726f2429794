// ell_sens_total.hip -- ell_sens_vs_total_kernel and bh_ell_sens_vs_total: the ellipticity kernel with vp tied to vs and
// rho to vp, per layer, in the operation order of sensitivity.vs_total.
//
// E depends on a layer through its vp / vs, so with vp = q vs the two parts of the total derivative cancel: at short
// periods K_vs and q K_vp of the top layer agree to seven digits and what is left is 1e-7 of either.  A difference like
// that is defined only together with the order of its roundings.  bh_sens_sets_add's BH_SENS_KIND_VS_TOTAL fuses the
// chain (two fma's), which is right for dc/dm and dU/dm, whose terms have one sign, and leaves this remainder 1e-9 away
// from what sensitivity.vs_total gives for the same K.  The ellipticity reduction therefore forms
//
//     G_l = K_vs,l + q_l (K_vp,l + drho_dvp K_rho,l)          each operation rounded once (-ffp-contract=off)
//
// here, bit for bit numpy's value, writes it where K_vs was, and hands the result to bh_sens_sets_add as
// BH_SENS_KIND_VS.  One lane per (model, period, layer): 3 loads and 1 store of 8 bytes.  A layer behind a model's last
// one gets whatever its q gives (NaN for 0 / 0); bh_sens_sets_add reads no such layer.
#include <hip/hip_runtime.h>
#include "../../include/bayhunter_amd.h"
#include "host_common.h"

namespace bh {

constexpr int ELL_SENS_TOTAL_T = 256;

__global__ __launch_bounds__(ELL_SENS_TOTAL_T) void ell_sens_vs_total_kernel(long npk, int nper, int Lmax, const double *K,
                                                                             const double *q, int q_stride, double drho_dvp,
                                                                             double *G)
{
    const long g = (long)blockIdx.x * ELL_SENS_TOTAL_T + threadIdx.x;
    if (g >= npk * Lmax) return;
    const long pk = g / Lmax;                        // (model, period)
    const int l = (int)(g - pk * Lmax);
    const long b = pk / nper;
    const double *Kp = K + pk * 4 * Lmax;
    const double t = Kp[Lmax + l] + drho_dvp * Kp[3 * Lmax + l];
    G[pk * 4 * Lmax + 2 * Lmax + l] = Kp[2 * Lmax + l] + q[b * q_stride + l] * t;
}

}  // namespace bh

extern "C" int bh_ell_sens_vs_total(int B, int Lmax, int nper, const double *K, const double *q, int q_stride, double drho_dvp,
                                    double *G, void *stream)
{
    if (B < 0 || Lmax < 1 || Lmax > BH_MAX_LAYERS) return bh::fail_arg_("B/Lmax out of range");
    if (nper < 1 || nper > BH_MAX_PERIODS) return bh::fail_arg_("nper out of range (1 .. 60)");
    if (q_stride < Lmax) return bh::fail_arg_("q_stride < Lmax");
    if (!K || !q || !G) return bh::fail_arg_("NULL pointer");
    if (B == 0) return BH_OK;
    const long npk = (long)B * nper, blocks = (npk * Lmax + bh::ELL_SENS_TOTAL_T - 1) / bh::ELL_SENS_TOTAL_T;
    if (blocks > 0x7fffffffL) return bh::fail_arg_("B * nper * Lmax lanes do not fit one launch");
    int rc = bh::require_device();
    if (rc) return rc;
    hipLaunchKernelGGL(bh::ell_sens_vs_total_kernel, dim3((unsigned)blocks), dim3(bh::ELL_SENS_TOTAL_T), 0, (hipStream_t)stream,
                       npk, nper, Lmax, K, q, q_stride, drho_dvp, G);
    BH_HIP(hipGetLastError());
    return BH_OK;
}
