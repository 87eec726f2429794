// posterior_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Compiles the per-row core of the posterior kernels (bayhunter_amd/csrc/posterior_core.h) with g++ so
// that the CPU tier replays the device arithmetic: Vs on the depth grid, interface depths, binning.
#define BH_HOSTSIM 1
#include "../../bayhunter_amd/csrc/posterior_core.h"

template <typename T>
static void interp_rows(const T *rows, long R, int width, const double *dep, int D, double *vs, int *n,
                        double *ifd)
{
    for (long r = 0; r < R; r++) {
        const T *row = rows + r * width;
        const int c = bh::post_row_count(row, width);
        n[r] = c / 2;
        for (int k = 0; k < width / 2; k++) ifd[r * (width / 2) + k] = __builtin_nan("");
        if (c < 2) {
            for (int d = 0; d < D; d++) vs[r * D + d] = __builtin_nan("");
            continue;
        }
        bh::PostWalk<T> wi;
        wi.init(row, c);
        for (int k = 0; wi.has_interface(); k++) {
            ifd[r * (width / 2) + k] = wi.D;
            wi.cross();
        }
        bh::PostWalk<T> wk;
        wk.init(row, c);
        for (int d = 0; d < D; d++) vs[r * D + d] = (double)wk.at(dep[d]);
    }
}

extern "C" void ps_interp32(const float *rows, long R, int width, const double *dep, int D, double *vs, int *n,
                            double *ifd)
{
    interp_rows(rows, R, width, dep, D, vs, n, ifd);
}
extern "C" void ps_interp64(const double *rows, long R, int width, const double *dep, int D, double *vs, int *n,
                            double *ifd)
{
    interp_rows(rows, R, width, dep, D, vs, n, ifd);
}
extern "C" void ps_bin(const double *edges, int ne, const double *v, long nv, int *out)
{
    for (long i = 0; i < nv; i++) out[i] = bh::post_bin(edges, ne, v[i]);
}
extern "C" void ps_keys(const double *v, long nv, unsigned long long *k64, double *back)
{
    for (long i = 0; i < nv; i++) {
        k64[i] = bh::post_key64(v[i]);
        back[i] = bh::post_unkey64(k64[i]);
    }
}
