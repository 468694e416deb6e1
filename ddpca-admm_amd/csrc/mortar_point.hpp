// Point arithmetic of the mortar operators (Interface::BUILD, mcontact.cpp: MCONTACT.h:181-810, with
// CONT_ROTA 157-179) shared by the host walk of the device path (mortar_host.cpp, device = -2) and
// the kernels (device_mortar.hip), so that both run the same operations in the same order.
// Interface::BUILD itself stays as it is and is the specification: every expression below is
// written as BUILD writes it, in the same loop order over m.  Plain inline functions: nothing here
// names a device symbol.
//
// * No contraction.  The host objects are x86-64 without FMA, so BUILD's `acc += mm * G` is a
//   multiply, then an add; the device compiler would fuse it.  Everything below is compiled with
//   fp contract(off) (the rule of csearch_face.hpp): the same mul, mul, add chains on gfx950 keep the
//   device at the host's bits.
// * One view, two memories.  MortarView holds raw pointers to one side's plan arrays (mortar_plan.hpp),
//   the points and the output values; the host walk fills it with host pointers, the launcher with
//   device pointers.  pair_lane / nodal_emit / inpo_emit / point_emit are the bodies of the kernels'
//   threads, and the host walk calls the very same functions.
// * Every loop is bounded by a count of the view and every write is checked against the length of
//   the array it goes to (put()).
#pragma once
#include <cstdint>

#include "stress_elem.hpp"  // DDPCA_HD

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ddpca {
namespace mortar {

// one integration point as 27 words of 8 bytes (IntegralPoint, mcontact.hpp): node[2][4] (int64),
// shap[2][4], basis[3][3], gap, w
constexpr int kPointWords = 27;
constexpr int kShap = 8, kBasis = 16, kGap = 25, kW = 26;

struct MortarView {
    int s = 0;  // side
    int64_t nip = 0, ncn = 0, npair = 0, ninc = 0;
    double pen[3] = {0.0, 0.0, 0.0};  // penN, penF, penF
    const double* pts = nullptr;       // kPointWords per point
    // the plan (mortar_plan.hpp, MortarSide)
    const int32_t* ipc = nullptr;
    const int32_t* inc_ptr = nullptr;
    const int32_t* inc = nullptr;
    const int32_t* inc_node = nullptr;
    const int32_t* pptr = nullptr;
    const int32_t* part = nullptr;
    const int32_t* pair_node = nullptr;
    const int32_t* byrank = nullptr;
    const int32_t* nrow0 = nullptr;
    const int32_t* rotidx = nullptr;
    const uint8_t* ord_c = nullptr;
    const uint8_t* ord_n = nullptr;
    const double* rot = nullptr;
    // the pair sums: aGP 9 per pair; aG 9 per pair (C = 3); aN 3 and aM 1 per pair (C = 1)
    double* aGP = nullptr;
    double* aG = nullptr;
    double* aN = nullptr;
    double* aM = nullptr;
    // the values of the nine operators and their lengths
    double* mass = nullptr;
    double* tran = nullptr;
    double* tranp = nullptr;
    double* imass = nullptr;
    double* imassp = nullptr;
    double* lagr = nullptr;
    double* disp = nullptr;
    double* inpo = nullptr;
    double* pema = nullptr;
    int64_t n_mass = 0, n_tran = 0, n_imass = 0, n_lagr = 0, n_disp = 0, n_inpo = 0;
};

DDPCA_HD void put(double* v, int64_t n, int64_t i, double x) {
    if (i >= 0 && i < n) v[i] = x;
}

// G = T^T T and GP = T^T P T over the first C rows of the basis (BUILD's x and y)
template <int C>
DDPCA_HD void point_G(const double* basis, const double (&pen)[3], double (&G)[3][3], double (&GP)[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double x = 0, y = 0;
            for (int m = 0; m < C; ++m) {
                x += basis[3 * m + i] * basis[3 * m + j];
                y += basis[3 * m + i] * pen[m] * basis[3 * m + j];
            }
            G[i][j] = x;
            GP[i][j] = y;
        }
}

// mm = w M_a M_b
DDPCA_HD double point_mm(double w, double Ma, double Mb) { return w * Ma * Mb; }

// CONT_ROTA on the three rows of a systTran(_pena) node: R^T o
DDPCA_HD void rota_rows(const double* R, const double (&o)[3], double (&v)[3]) {
    for (int a = 0; a < 3; ++a) v[a] = R[a] * o[0] + R[3 + a] * o[1] + R[6 + a] * o[2];
}
// CONT_ROTA on a node's three inpoDisp columns: o R
DDPCA_HD void rota_cols(const double* R, const double (&o)[3], double (&v)[3]) {
    for (int b = 0; b < 3; ++b) v[b] = o[0] * R[b] + o[1] * R[3 + b] + o[2] * R[6 + b];
}

// the entry values of the per-point operators
template <int C>
DDPCA_HD double lagr_value(const double* basis, const double* M, int m, int a, int k) {
    return C == 1 ? M[a] : basis[3 * m + k] * M[a];
}
template <int C>
DDPCA_HD double disp_value(const double* basis, const double* M, int m, int an, int k) {
    return basis[3 * (C == 1 ? 0 : m) + k] * M[an];
}
template <int C>
DDPCA_HD double inpo_value(double sgn, double w, const double* basis, const double* M, int m, int a, int k) {
    return sgn * (w * M[a] * (C == 1 ? 1.0 : basis[3 * m + k]));
}

// ---- k_mortar_pair: the sums of pair (c, its partner of rank t), over c's incidence list in order
// (q, then a), then b: the order BUILD adds them in
template <int C>
DDPCA_HD void pair_lane(const MortarView& V, int32_t c, int32_t t) {
    const int32_t k = V.pptr[c] + t;
    if (k < 0 || k >= V.npair) return;
    const int32_t cb = V.part[k];
    double aGP[9], aG[9], aN[3], aM = 0.0;
    for (int i = 0; i < 9; ++i) aGP[i] = 0.0, aG[i] = 0.0;
    for (int i = 0; i < 3; ++i) aN[i] = 0.0;
    int32_t e0 = V.inc_ptr[c], e1 = V.inc_ptr[c + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > V.ninc) e1 = (int32_t)V.ninc;
    for (int32_t e = e0; e < e1; ++e) {
        const int32_t qa = V.inc[e];
        const int64_t q = qa >> 2;
        const int a = qa & 3;
        if (q < 0 || q >= V.nip) continue;
        const int32_t* pc = V.ipc + 4 * q;
        const bool h0 = pc[0] == cb, h1 = pc[1] == cb, h2 = pc[2] == cb, h3 = pc[3] == cb;
        if (!(h0 || h1 || h2 || h3)) continue;
        const double* P = V.pts + kPointWords * q;
        const double* M = P + kShap + 4 * V.s;
        const double* basis = P + kBasis;
        double GP[3][3], G[3][3];
        point_G<C>(basis, V.pen, G, GP);
        for (int b = 0; b < 4; ++b) {
            if (!(b == 0 ? h0 : b == 1 ? h1 : b == 2 ? h2 : h3)) continue;
            const double mm = point_mm(P[kW], M[a], M[b]);
            for (int u = 0; u < 9; ++u) {
                aGP[u] += mm * GP[u / 3][u % 3];
                if (C == 3) aG[u] += mm * G[u / 3][u % 3];
            }
            if (C == 1) {
                for (int i = 0; i < 3; ++i) aN[i] += mm * basis[i];
                aM += mm;
            }
        }
    }
    for (int u = 0; u < 9; ++u) {
        V.aGP[9 * (int64_t)k + u] = aGP[u];
        if (C == 3) V.aG[9 * (int64_t)k + u] = aG[u];
    }
    if (C == 1) {
        for (int i = 0; i < 3; ++i) V.aN[3 * (int64_t)k + i] = aN[i];
        V.aM[k] = aM;
    }
}

// ---- k_mortar_nodal: pair k's values of systMass (through bypos), systTran(_pena) (rotated where
// the row's node has a rotation) and inteMass(_pena), at BUILD's positions
template <int C>
DDPCA_HD void nodal_emit(const MortarView& V, int64_t k) {
    if (k < 0 || k >= V.npair) return;
    const int32_t a = V.pair_node[k];
    if (a < 0 || a >= V.ncn) return;
    const int64_t np = V.pptr[a + 1] - V.pptr[a], t = k - V.pptr[a], tt = V.byrank[k];
    const int64_t r0 = V.nrow0[a];
    const double* R = V.rotidx[a] >= 0 ? V.rot + 9 * (int64_t)V.rotidx[a] : nullptr;
    const double penN = V.pen[0];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) put(V.mass, V.n_mass, 9 * r0 + i * 3 * np + 3 * tt + j, V.aGP[9 * k + 3 * i + j]);
    if (C == 3) {
        for (int j = 0; j < 3; ++j) {
            double o[3] = {V.aG[9 * k + j], V.aG[9 * k + 3 + j], V.aG[9 * k + 6 + j]};
            double op[3] = {V.aGP[9 * k + j], V.aGP[9 * k + 3 + j], V.aGP[9 * k + 6 + j]};
            if (R) {
                double v[3];
                rota_rows(R, o, v);
                for (int i = 0; i < 3; ++i) o[i] = v[i];
                rota_rows(R, op, v);
                for (int i = 0; i < 3; ++i) op[i] = v[i];
            }
            for (int i = 0; i < 3; ++i) {
                put(V.tran, V.n_tran, 9 * r0 + i * 3 * np + 3 * t + j, o[i]);
                put(V.tranp, V.n_tran, 9 * r0 + i * 3 * np + 3 * t + j, op[i]);
            }
        }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const int64_t w = 9 * (int64_t)V.pptr[a] + i * 3 * np + 3 * t + j;
                put(V.imass, V.n_imass, w, V.aG[9 * k + 3 * i + j]);
                put(V.imassp, V.n_imass, w, V.aGP[9 * k + 3 * i + j]);
            }
    } else {
        double o[3] = {V.aN[3 * k], V.aN[3 * k + 1], V.aN[3 * k + 2]};
        double op[3] = {penN * V.aN[3 * k], penN * V.aN[3 * k + 1], penN * V.aN[3 * k + 2]};
        if (R) {
            double v[3];
            rota_rows(R, o, v);
            for (int i = 0; i < 3; ++i) o[i] = v[i];
            rota_rows(R, op, v);
            for (int i = 0; i < 3; ++i) op[i] = v[i];
        }
        for (int i = 0; i < 3; ++i) {
            put(V.tran, V.n_tran, 3 * r0 + i * np + t, o[i]);
            put(V.tranp, V.n_tran, 3 * r0 + i * np + t, op[i]);
        }
        put(V.imass, V.n_imass, k, V.aM[k]);
        put(V.imassp, V.n_imass, k, V.aM[k] * penN);
    }
}

// ---- k_mortar_ip, first kind: position e of the incidence lists, entry (q, a) of rank r in node c's
// list, writes its C x C values of inteInpo at ptr[C c + k] + C r + m
template <int C>
DDPCA_HD void inpo_emit(const MortarView& V, int64_t e) {
    if (e < 0 || e >= V.ninc) return;
    const int32_t c = V.inc_node[e], qa = V.inc[e];
    const int64_t q = qa >> 2;
    const int a = qa & 3;
    if (c < 0 || c >= V.ncn || q < 0 || q >= V.nip) return;
    const int64_t cnt = V.inc_ptr[c + 1] - V.inc_ptr[c], r = e - V.inc_ptr[c];
    const double* P = V.pts + kPointWords * q;
    const double* M = P + kShap + 4 * V.s;
    const double sgn = (V.s == 0) ? -1.0 : 1.0;
    for (int k = 0; k < C; ++k)
        for (int m = 0; m < C; ++m)
            put(V.inpo, V.n_inpo, (int64_t)C * C * V.inc_ptr[c] + k * C * cnt + C * r + m,
                inpo_value<C>(sgn, P[kW], P + kBasis, M, m, a, k));
}

// ---- k_mortar_ip, second kind: point q writes its C rows of inpoLagr, inpoDisp (a node's three
// columns rotated where it has a rotation) and pemaInpo_r = pemaDiag inpoDisp, through ord_c / ord_n
template <int C>
DDPCA_HD void point_emit(const MortarView& V, int64_t q) {
    if (q < 0 || q >= V.nip) return;
    const double* P = V.pts + kPointWords * q;
    const double* M = P + kShap + 4 * V.s;
    const double* basis = P + kBasis;
    for (int m = 0; m < C; ++m) {
        const int64_t r = C * q + m;
        int64_t wl = 4 * C * r, wd = 12 * r;
        for (int t = 0; t < 4; ++t) {
            const int a = V.ord_c[4 * q + t] & 3;
            if (C == 1) {
                put(V.lagr, V.n_lagr, wl++, lagr_value<C>(basis, M, m, a, 0));
            } else {
                for (int k = 0; k < 3; ++k) put(V.lagr, V.n_lagr, wl++, lagr_value<C>(basis, M, m, a, k));
            }
            const int an = V.ord_n[4 * q + t] & 3;
            double o[3];
            for (int k = 0; k < 3; ++k) o[k] = disp_value<C>(basis, M, m, an, k);
            const int32_t cn = V.ipc[4 * q + an];
            const int32_t ri = (cn >= 0 && cn < V.ncn) ? V.rotidx[cn] : -1;
            if (ri >= 0) {
                double v[3];
                rota_cols(V.rot + 9 * (int64_t)ri, o, v);
                for (int k = 0; k < 3; ++k) o[k] = v[k];
            }
            for (int k = 0; k < 3; ++k) {
                put(V.disp, V.n_disp, wd, o[k]);
                put(V.pema, V.n_disp, wd, o[k] * V.pen[m]);
                ++wd;
            }
        }
    }
}

}  // namespace mortar
}  // namespace ddpca
