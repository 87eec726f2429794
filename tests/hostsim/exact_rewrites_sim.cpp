// exact_rewrites_sim.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_swd_exact_rewrites.py, tests/test_gpu_exact_rewrites.py).
// 1. The expressions of the Rayleigh / Love layer step that were rewritten as explicit fusions with an exact factor
//    (bh_common.h: bh_fma_exact2), each beside the form it had before, operand by operand.
// 2. The period table of swd_kernel (swd_core.h: SwdPerTab) beside the divisions at the event that it replaces.
// 3. The loop of swd_lane over a batch of models, reading the periods from the table (what swd_kernel runs) or
//    directly (what the team kernels run).
// Built as a shared library, or with -DER_MAIN as a program of its own (the sanitizer run: it reads a batch from a
// file, replays it with both period sources and compares).
#define BH_HOSTSIM 1
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../bayhunter_amd/csrc/swd_core.h"

namespace {
struct HostLay {
    float *pd, *pa, *pb, *pr;
    float d(int i) const { return pd[i]; }
    float a(int i) const { return pa[i]; }
    float b(int i) const { return pb[i]; }
    float rho(int i) const { return pr[i]; }
    void set_d(int i, float v) { pd[i] = v; }
    void set_a(int i, float v) { pa[i] = v; }
    void set_b(int i, float v) { pb[i] = v; }
    void set_rho(int i, float v) { pr[i] = v; }
};
struct OneTask {
    HostLay src;
    int nlayer, taken, err;
    double *out, *cws, *cbws;
    int next(HostLay &lay, double *&o, double *&c, double *&cb)
    {
        if (taken) return 0;
        taken = 1;
        lay = src;
        o = out; c = cws; cb = cbws;
        return nlayer;
    }
    void done(int e) { err = e; }
    void sphere(HostLay &lay, int mmax, int ifunc) { bh::swd_sphere(lay, mmax, ifunc); }
    void put(bh::SwdState &S, int k, int kmax, float v) { bh::swd_put_direct(S, k, kmax, v); }
    void fill_zero(bh::SwdState &S, int k, int kmax) { bh::swd_zero_direct(S, k, kmax); }
};
}  // namespace

// which: 0 cos of the evanescent arm, (1 + a) * 0.5          1 sin, (1 - a) * 0.5
//        2 c11's head, a - 2 * b * c                          3 c15's head, 2 * a * b + c
//        4 c51's head, 2 * a * b * c + d                      5 c33, a + 2 * (b - c)
// The `before` forms are the expressions of the parent as they stood (compiled with -ffp-contract=off).
extern "C" void er_forms(int which, long n, const double *a, const double *b, const double *c, const double *d,
                         double *before, double *after)
{
    const double two = 2.0;
    for (long i = 0; i < n; i++) {
        switch (which) {
        case 0: before[i] = (1.0 + a[i]) * 0.5; after[i] = bh::bh_fma_exact2(a[i], 0.5, 0.5); break;
        case 1: before[i] = (1.0 - a[i]) * 0.5; after[i] = bh::bh_fma_exact2(-a[i], 0.5, 0.5); break;
        case 2: before[i] = a[i] - two * b[i] * c[i]; after[i] = bh::bh_fma_exact2(b[i] * c[i], -two, a[i]); break;
        case 3: before[i] = two * a[i] * b[i] + c[i]; after[i] = bh::bh_fma_exact2(a[i] * b[i], two, c[i]); break;
        case 4: before[i] = two * a[i] * b[i] * c[i] + d[i]; after[i] = bh::bh_fma_exact2(a[i] * b[i] * c[i], two, d[i]); break;
        default: before[i] = a[i] + two * (b[i] - c[i]); after[i] = bh::bh_fma_exact2(b[i] - c[i], two, a[i]); break;
        }
    }
}

// Period k0 (0-based) of `per`: table[4] = oma, omb, t1a, t1b as swd_pertab_put stores and the events read them;
// event[4] = the same four as the events work them out from the periods (first solve, then the second of the pair).
extern "C" void er_period(const double *per, int n, int k0, int igr, double *table, double *event)
{
    std::vector<double> tab(bh::swd_pertab_doubles(n, igr > 0) + 1, -1.0);
    for (int k = 0; k < n; k++) bh::swd_pertab_put(tab.data(), n, k, per[k], igr);
    const bh::SwdPerTab T{tab.data(), n};
    const bh::SwdTargetDev tg{2, igr, 1, 0, n, 0, 0, 0};
    bh::SwdState S, D;
    bh::swd_state_init(S);
    bh::swd_state_init(D);
    S.k = D.k = k0 + 1;
    table[0] = bh::swd_period_begin(S, tg, T);
    table[1] = igr > 0 ? bh::swd_period_second(S, T) : 0.0;
    table[2] = igr > 0 ? (double)bh::swd_period_t1a(S, T) : (double)(float)per[k0];
    table[3] = igr > 0 ? (double)bh::swd_period_t1b(S, T) : 0.0;
    event[0] = bh::swd_period_begin(D, tg, per);
    event[1] = igr > 0 ? bh::swd_period_second(D, per) : 0.0;
    event[2] = (double)bh::swd_period_t1a(D, per);
    event[3] = igr > 0 ? (double)bh::swd_period_t1b(D, per) : 0.0;
}

// The divisions as the parent wrote them at the events (surfdisp96.f:233-240, 283): out[4] = oma, omb, t1a, t1b.
extern "C" void er_period_before(double t1, int igr, double *out)
{
    const double TWOPI = 2.0 * 3.141592653589793;
    const float h = 0.005f;
    float t1a, t1b = 0.f;
    double t = t1;
    if (igr > 0) {
        t1a = (float)(t / (double)(1.f + h));
        t1b = (float)(t / (double)(1.f - h));
        t = (double)t1a;
    } else {
        t1a = (float)t;
    }
    out[0] = TWOPI / t;
    out[1] = igr > 0 ? TWOPI / (double)t1b : 0.0;
    out[2] = (double)t1a;
    out[3] = (double)t1b;
}

// swd_lane over B models ([B][Lmax] fp64 arrays holding fp32 values, nl layers each).  table != 0: the periods come
// from a SwdPerTab.  cg [B][nper], err [B].
extern "C" int er_batch(int B, int Lmax, const double *H, const double *VP, const double *VS, const double *RHO,
                        const int *nl, int iflsph, int iwave, int mode, int igr, int nper, const double *per,
                        int table, double *cg, int *err)
{
    std::vector<double> tab(bh::swd_pertab_doubles(nper, igr > 0) + 1, 0.0);
    for (int k = 0; k < nper; k++) bh::swd_pertab_put(tab.data(), nper, k, per[k], igr);
    const bh::SwdPerTab T{tab.data(), nper};
    const bh::SwdTargetDev tg{iwave, igr, mode, iflsph, nper, 0, 0, 0};
    for (int b = 0; b < B; b++) {
        const int n = nl[b];
        if (n < 1 || n > Lmax) return 1;
        std::vector<float> d(n), a(n), s(n), r(n);
        for (int l = 0; l < n; l++) {
            d[l] = (float)H[(long)b * Lmax + l]; a[l] = (float)VP[(long)b * Lmax + l];
            s[l] = (float)VS[(long)b * Lmax + l]; r[l] = (float)RHO[(long)b * Lmax + l];
        }
        std::vector<double> cws(nper > 0 ? nper : 1), cbws(nper > 0 ? nper : 1);
        HostLay lay{nullptr, nullptr, nullptr, nullptr};
        OneTask src{HostLay{d.data(), a.data(), s.data(), r.data()}, n, 0, -1, cg + (long)b * nper, cws.data(), cbws.data()};
        if (table) bh::swd_lane(lay, src, tg, T, 1, nullptr);
        else bh::swd_lane(lay, src, tg, per, 1, nullptr);
        err[b] = src.err;
    }
    return 0;
}

#if defined(ER_MAIN)
// file: int32 B, Lmax, nper; then H, VP, VS, RHO [B][Lmax] fp64, per [nper] fp64, nl [B] int32
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[3];
    if (fread(hdr, sizeof(int), 3, f) != 3) return 2;
    const int B = hdr[0], L = hdr[1], np = hdr[2];
    std::vector<double> m[4], per(np);
    for (auto &x : m) {
        x.resize((size_t)B * L);
        if (fread(x.data(), sizeof(double), x.size(), f) != x.size()) return 2;
    }
    std::vector<int> nl(B);
    if (fread(per.data(), sizeof(double), np, f) != (size_t)np || fread(nl.data(), sizeof(int), B, f) != (size_t)B) return 2;
    fclose(f);
    long bad = 0, vals = 0;
    const int targets[4][3] = {{2, 0, 1}, {2, 1, 2}, {1, 0, 1}, {1, 1, 1}};      // iwave, igr, modes
    for (const auto &t : targets) {
        std::vector<double> c0((size_t)B * np), c1((size_t)B * np);
        std::vector<int> e0(B), e1(B);
        if (er_batch(B, L, m[0].data(), m[1].data(), m[2].data(), m[3].data(), nl.data(), 0, t[0], t[2], t[1], np,
                     per.data(), 1, c0.data(), e0.data()) ||
            er_batch(B, L, m[0].data(), m[1].data(), m[2].data(), m[3].data(), nl.data(), 0, t[0], t[2], t[1], np,
                     per.data(), 0, c1.data(), e1.data()))
            return 3;
        bad += memcmp(c0.data(), c1.data(), c0.size() * sizeof(double)) != 0;
        bad += memcmp(e0.data(), e1.data(), e0.size() * sizeof(int)) != 0;
        vals += (long)c0.size();
    }
    printf("replayed %d models x 4 targets, %ld values, table and direct period sources differ in %ld arrays\n", B, vals, bad);
    return bad ? 1 : 0;
}
#endif
