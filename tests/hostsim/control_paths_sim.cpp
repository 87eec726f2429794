// control_paths_sim.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_gpu_control_paths.py).
// The throughput kernel's loop (swd_events_pass, period equation, swd_control for a table in registers) run
// model by model on the CPU, with counters of the paths the control code and the event pass take, and with the
// generic swd_control (table in memory) running beside it on a copy of the state: the two must leave the same
// state and the same table after every evaluation.  Never loaded by the bayhunter_amd package.
#define BH_HOSTSIM 1
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
bool same(double a, double b) { return a == b || (a != a && b != b); }
}  // namespace

// counters, per model
enum {
    CP_POINTS0 = 0,        // [p], p = 2 .. 11: Neville passes that succeeded on a table of p points
    CP_GUARD = 12,         // Neville passes whose guard fired (-> bisection)
    CP_TURN = 13,          // bracketing steps that turned round at clow
    CP_NOROOT1 = 14,       // searches that ended without a root on the first solve
    CP_NOROOT2 = 15,       // ... on the second solve of a group-velocity pair
    CP_LEFTOVER = 16,      // event passes that left an event pending (the lane sits out a trip)
    CP_MODE2 = 17,         // evaluations in a mode above the fundamental
    CP_EVALS = 18,
    CP_TOMID = 19,         // Neville estimates outside the bracket (-> midpoint, state MID)
    CP_N = 24
};

// returns 0, or -200 when the flat and the generic control code part ways
extern "C" int cp_batch(int B, int Lmax, const double *h, const double *vp, const double *vs, const double *rho,
                        const int *nlay, int iflsph, int iwave, int mode, int igr, int kmax, const double *t,
                        double *cg, int *err, long *cnt)
{
    const double pct = (double)0.01f;               // `0.01` literal in nevill is real*4
    for (int bi = 0; bi < B; bi++) {
        const int nl = nlay[bi];
        std::vector<float> d(nl), a(nl), b(nl), r(nl);
        for (int i = 0; i < nl; i++) {
            d[i] = (float)h[(long)bi * Lmax + i]; a[i] = (float)vp[(long)bi * Lmax + i];
            b[i] = (float)vs[(long)bi * Lmax + i]; r[i] = (float)rho[(long)bi * Lmax + i];
        }
        long *c = cnt + (long)bi * CP_N;
        for (int i = 0; i < CP_N; i++) c[i] = 0;
        HostLay lay{nullptr, nullptr, nullptr, nullptr};
        bh::SwdTargetDev tg{iwave, igr, mode, iflsph, kmax, 0, 0, 0};
        std::vector<double> cws(kmax > 0 ? kmax : 1), cbws(kmax > 0 ? kmax : 1);
        OneTask src{HostLay{d.data(), a.data(), b.data(), r.data()}, nl, 0, -1, cg + (long)bi * kmax, cws.data(),
                    cbws.data()};
        bh::SwdState S;
        bh::swd_state_init(S);
        bh::NevRegs nv;
        bh::swd_nev_init(nv);
        double gx[12], gy[12];
        bh::NevMem gv{gx, gy};
        bh::swd_nev_init(gv);
        for (;;) {
            bh::swd_events_pass(S, lay, src, tg, t, 1);
            if (S.ev != bh::SWD_EV_NONE) { c[CP_LEFTOVER]++; continue; }
            if (S.st == bh::SWD_ST_DONE) break;
            const double wvno = S.omega / S.ceval;
            const double del = (iwave == 1) ? bh::swd_dltar1(lay, S.mmax, S.llw, wvno, S.omega)
                                            : bh::swd_dltar4(lay, S.mmax, S.llw, wvno, S.omega);
            c[CP_EVALS]++;
            if (S.iq > 1) c[CP_MODE2]++;
            // what the reference's code is about to do, from the state as it is (surfdisp96.f:587-669)
            const bh::SwdState P = S;
            bool to_neville = false;
            if (P.st == bh::SWD_ST_TOP || P.st == bh::SWD_ST_MID) {
                bool mid = P.st == bh::SWD_ST_MID, fin = false;
                if (!mid) {
                    if (P.nctrl + 1 >= 100) fin = true;
                    else if (P.c3 < bh::dmin(P.c1, P.c2) || P.c3 > bh::dmax(P.c1, P.c2)) c[CP_TOMID]++;
                    else mid = true;
                }
                if (mid && !fin) {
                    const bool hi = bh::bh_signs_differ(del, P.del1);
                    const double c1 = hi ? P.c1 : P.c3, d1 = hi ? P.del1 : del;
                    const double c2 = hi ? P.c3 : P.c2, d2 = hi ? del : P.del2;
                    if (!(fabs(c1 - c2) <= 1.e-6 * c1)) {
                        const int nev = bh::bh_signs_differ(P.del1 - del, del - P.del2) ? 0 : P.nev;
                        const double ss1 = fabs(d1), ss2 = fabs(d2);
                        to_neville = !(pct * ss1 > ss2 || pct * ss2 > ss1 || nev == 0);
                    }
                }
            }
            int want_idir = P.idir;
            if (P.st == bh::SWD_ST_A) want_idir = (P.ifirst == 1 || !bh::bh_signs_differ(P.del1st, del)) ? +1 : -1;
            bh::SwdState G = S;
            bh::swd_control(S, del, nv);
            bh::swd_control(G, del, gv);
            // the flat form against the generic one: state and table
            const double fx[12] = {0, nv.x1, nv.x2, nv.x3, nv.x4, nv.x5, nv.x6, nv.x7, nv.x8, nv.x9, nv.x10, nv.x11};
            const double fy[12] = {0, nv.y1, nv.y2, nv.y3, nv.y4, nv.y5, nv.y6, nv.y7, nv.y8, nv.y9, nv.y10, nv.y11};
            bool eq = G.st == S.st && G.ev == S.ev && G.nev == S.nev && G.m == S.m && G.nctrl == S.nctrl &&
                      G.idir == S.idir && G.nbrk == S.nbrk && same(G.c1, S.c1) && same(G.c2, S.c2) &&
                      same(G.c3, S.c3) && same(G.del1, S.del1) && same(G.del2, S.del2) && same(G.del3, S.del3) &&
                      same(G.del1st, S.del1st) && same(G.ceval, S.ceval) && same(G.clow, S.clow);
            for (int i = 1; i < 12; i++) eq = eq && same(fx[i], gx[i]) && same(fy[i], gy[i]);
            if (!eq) return -200;
            if (to_neville) {
                if (S.nev == 2) {
                    const int steps = P.nev == 2 ? P.m : 1;      // append to m points, or restart from the ends
                    c[CP_POINTS0 + steps + 1]++;
                } else c[CP_GUARD]++;
            }
            if (S.st == bh::SWD_ST_B && S.ev == bh::SWD_EV_NONE && (P.st == bh::SWD_ST_A || P.st == bh::SWD_ST_B) &&
                want_idir < 0 && S.idir > 0)
                c[CP_TURN]++;
            if (S.ev == bh::SWD_EV_NOROOT) c[S.pass == 1 ? CP_NOROOT2 : CP_NOROOT1]++;
        }
        err[bi] = src.err;
    }
    return 0;
}
