// CPU replay of like_gaps_kernel's closed forms for a block of rows: the staging of the residuals through each
// set's column list, every lane's share of the sums, the butterfly of wave_sum and the target's figures -- the very
// functions of bayhunter_amd/csrc/like_core.h that like_kernel.hip compiles for the device, with the same
// lane-to-element numbering, on a host array in place of LDS.  present == null replays the unmasked form (n' = n).
// Built by tests/test_station_gaps.py with g++ and glibc math (-ffp-contract=off).
#define BH_HOSTSIM 1
#include <cmath>
#include <vector>
#include "../../bayhunter_amd/csrc/like_core.h"

using namespace bh;

namespace {
struct Tg { int n, off, cov; };

double wave_sum(double *v)            // like_kernel.hip: v += __shfl_xor(v, o, 64) for o = 32 .. 1, on all 64 lanes
{
    for (int o = 32; o > 0; o >>= 1) {
        double w[64];
        for (int l = 0; l < 64; l++) w[l] = v[l] + v[l ^ o];
        for (int l = 0; l < 64; l++) v[l] = w[l];
    }
    return v[0];
}

template <bool MASKED>
void replay(int M, int T, const Tg *tg, const double *extra, const double *out, int out_stride, const int *obs_id,
            const double *yobs, int set_stride, const double *set_scale, const double *set_logdet, const double *noise,
            const int *cols, const int *cnt, double *logL, double *misfits)
{
    for (int m = 0; m < M; m++) logL[m] = misfits[(long)m * (T + 1) + T] = 0.0;
    for (int t = 0; t < T; t++) {
        const int n = tg[t].n, off = tg[t].off;
        std::vector<double> sm((size_t)M * n, NAN);                       // the workgroup's LDS image, pitch n
        for (int idx = 0; idx < M * n; idx++) {
            const int m = idx / n, i = idx - m * n, set = obs_id ? obs_id[m] : 0;
            if (MASKED && i >= cnt[(long)set * T + t]) continue;
            sm[(size_t)m * n + i] = like_residual<MASKED>(out + (long)m * out_stride + off, yobs + (long)set * set_stride + off,
                                                          MASKED ? cols + (long)set * set_stride + off : nullptr, i);
        }
        for (int m = 0; m < M; m++) {
            const int set = obs_id ? obs_id[m] : 0;
            const int nk = MASKED ? cnt[(long)set * T + t] : n;
            const double *d = sm.data() + (size_t)m * n;
            const double corr = noise[(long)m * 2 * T + 2 * t], sigma = noise[(long)m * 2 * T + 2 * t + 1];
            double s2[64], q[64];
            for (int lane = 0; lane < 64; lane++) {
                s2[lane] = q[lane] = 0.0;
                if (tg[t].cov == 0) like_nocorr_lane(d, nk, lane, s2[lane], q[lane]);
                else if (tg[t].cov == 1)
                    like_scaled_lane<MASKED>(d, nk, lane, set_scale + (long)set * set_stride + off,
                                             MASKED ? cols + (long)set * set_stride + off : nullptr, s2[lane], q[lane]);
                else like_exp_lane(d, nk, lane, corr, s2[lane], q[lane]);
            }
            double logl, rms;
            like_target_part(tg[t].cov, nk, wave_sum(s2), wave_sum(q), corr, sigma,
                             tg[t].cov == 1 ? set_logdet[(long)set * T + t] : extra[t], logl, rms);
            logL[m] += logl;
            misfits[(long)m * (T + 1) + t] = rms;
            misfits[(long)m * (T + 1) + T] += rms;
        }
    }
}
}  // namespace

// targets: [T][3] ints (n, off, cov: 0, 1 or 2 -- the closed forms), extra[T]; out[M][out_stride]; obs_id[M] or null;
// yobs, set_scale [nsets][set_stride]; set_logdet[nsets][T]; noise[M][2T]; present[nsets][set_stride] bytes or null.
// Returns like_gap_tables' code (0; 1: dense target with a gap; 2: empty target), set and target in bad[2].
extern "C" int hs_like_gaps(int M, int T, const int *targets, const double *extra, const double *out, int out_stride,
                            int nsets, const int *obs_id, const double *yobs, int set_stride, const double *set_scale,
                            const double *set_logdet, const double *noise, const unsigned char *present, double *logL,
                            double *misfits, int *bad)
{
    std::vector<Tg> tg(T);
    for (int t = 0; t < T; t++) tg[t] = Tg{targets[3 * t], targets[3 * t + 1], targets[3 * t + 2]};
    if (!present) {
        replay<false>(M, T, tg.data(), extra, out, out_stride, obs_id, yobs, set_stride, set_scale, set_logdet, noise, nullptr,
                      nullptr, logL, misfits);
        return 0;
    }
    std::vector<int> cols((size_t)nsets * set_stride), cnt((size_t)nsets * T);
    bool any = false;
    const int rc = like_gap_tables(nsets, set_stride, T, tg.data(), present, cols.data(), cnt.data(), &any, &bad[0], &bad[1]);
    if (rc) return rc;
    replay<true>(M, T, tg.data(), extra, out, out_stride, obs_id, yobs, set_stride, set_scale, set_logdet, noise, cols.data(),
                 cnt.data(), logL, misfits);
    return 0;
}
