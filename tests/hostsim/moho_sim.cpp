// moho_sim.cpp -- TEST INFRASTRUCTURE ONLY.
// Compiles the per-row core of the Moho kernels (bayhunter_amd/csrc/moho_core.h) with g++ so that the CPU tier
// replays the device arithmetic against the numpy restatement (tests/moho_ref.py).
#define BH_HOSTSIM 1
#include "../../bayhunter_amd/csrc/moho_core.h"

template <typename T>
static long derive_rows(const T *rows, long R, long stride, int width, double zlo, double zhi, double mohovs, double *out)
{
    long found = 0;
    for (long r = 0; r < R; r++) found += bh::moho_row(rows + r * stride, width, zlo, zhi, mohovs, out + 4 * r);
    return found;
}

extern "C" long ms_rows32(const float *rows, long R, long stride, int width, double zlo, double zhi, double mohovs,
                          double *out)
{
    return derive_rows(rows, R, stride, width, zlo, zhi, mohovs, out);
}
extern "C" long ms_rows64(const double *rows, long R, long stride, int width, double zlo, double zhi, double mohovs,
                          double *out)
{
    return derive_rows(rows, R, stride, width, zlo, zhi, mohovs, out);
}
