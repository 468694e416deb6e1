// Face-pair arithmetic of the contact search (SI_SUB / SEGMENT_INTERSECT, CSEARCH.h:614-775, with
// PROJECT_MTS 232-307, PROJECT_STM 309-428, IS_CROSS_2D / LINE_INTERSECT_2D 495-597, IN_CQUAD_2D
// 599-612) shared by the host two-pass path (csearch.cpp, device = -2) and the device kernels
// (device_csearch.hip), so that both run the same operations in the same order.  It restates the
// per-pair functions of csearch.cpp without std::vector, std::sort or recursion; csearch.cpp's own
// functions (the default host search) stay as they are and are the specification.  Plain inline
// functions: nothing here names a device symbol.
//
// * No contraction.  The host objects are x86-64 without FMA; the device compiler would fuse
//   a * b - c * d.  The clip's decisions sit on exact zeros when faces coincide (straddle <= 0, the
//   1e-12 area tests, the 1e-10 de-duplication), so everything below is compiled with
//   fp contract(off): the one place in the library where explicit fma chains are wrong.  (The
//   pragma stays in force for the rest of a translation unit that includes this header.)
// * Fixed capacities.  The clip list holds at most 4 + 4 corners inside the other quad and 2 points
//   for each of the 16 edge pairs: kMaxClip = 40.  The polygon has at most as many vertices and a
//   pair at most 4 * 40 = 160 quadrature points.
// * The clip list, the polygon and the vertex angles live in caller-provided storage (Slots): three
//   arrays of kMaxClip doubles, element i at [i * stride] -- per-thread LDS columns on the device,
//   a local array (stride 1) on the host.  The slave corners' projections borrow the first 8 angle
//   slots: the clip is finished with them before the angles are written.
// * The two sorts are stable insertion sorts in place.  They may differ from std::sort only in
//   which member of a cluster of points equal within 1e-10 survives the de-duplication.
// * Every loop is bounded: the Newton loops by 60, the stepped approach of PROJECT_STM by `cap`
//   (the caller's bound, never reached on input that passed csearch_check).
#pragma once
#include <cmath>

#include "stress_elem.hpp"  // DDPCA_HD

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ddpca {
namespace csface {

constexpr int kMaxClip = 40;              // 4 + 4 + 16 * 2
constexpr int kMaxPoints = 4 * kMaxClip;  // per face pair
static_assert(kMaxClip == 4 + 4 + 16 * 2, "clip list bound");
constexpr double kMiniArea = 1.0e-12;     // CSEARCH.h:12

struct Slots {
    double* x;
    double* y;
    double* a;
    int stride;
};

// biliQuad.nacoCorn: corner k of the reference quad
DDPCA_HD double corn_x(int k) { return (k == 1 || k == 2) ? 1.0 : -1.0; }
DDPCA_HD double corn_y(int k) { return k >= 2 ? 1.0 : -1.0; }

DDPCA_HD double dot3(const double (&a)[3], const double (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
DDPCA_HD void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
DDPCA_HD void normalized(const double (&a)[3], double (&o)[3]) {
    const double n = sqrt(dot3(a, a));
    o[0] = a[0] / n, o[1] = a[1] / n, o[2] = a[2] / n;
}
DDPCA_HD double dmin(double a, double b) { return b < a ? b : a; }  // std::min / std::max
DDPCA_HD double dmax(double a, double b) { return a < b ? b : a; }

// 2x2 solve with full pivoting; the pivot search in csearch.cpp's order ((0,0), (0,1), (1,0), (1,1),
// a later entry wins only when strictly larger)
DDPCA_HD void solve2(double a00, double a01, double a10, double a11, double b0, double b1, double& x0, double& x1) {
    int pr = 0, pc = 0;
    double amax = -1.0;
    if (fabs(a00) > amax) amax = fabs(a00), pr = 0, pc = 0;
    if (fabs(a01) > amax) amax = fabs(a01), pr = 0, pc = 1;
    if (fabs(a10) > amax) amax = fabs(a10), pr = 1, pc = 0;
    if (fabs(a11) > amax) amax = fabs(a11), pr = 1, pc = 1;
    if (amax == 0.0) {
        x0 = x1 = 0.0;
        return;
    }
    // A[pr][pc], A[pr][qc], A[qr][pc], A[qr][qc] and b[pr], b[qr]
    const double app = pr == 0 ? (pc == 0 ? a00 : a01) : (pc == 0 ? a10 : a11);
    const double apq = pr == 0 ? (pc == 0 ? a01 : a00) : (pc == 0 ? a11 : a10);
    const double aqp = pr == 0 ? (pc == 0 ? a10 : a11) : (pc == 0 ? a00 : a01);
    const double aqq = pr == 0 ? (pc == 0 ? a11 : a10) : (pc == 0 ? a01 : a00);
    const double bp = pr == 0 ? b0 : b1, bq = pr == 0 ? b1 : b0;
    const double l = aqp / app;
    const double u = aqq - l * apq;
    const double y = bq - l * bp;
    const double xq = u != 0.0 ? y / u : 0.0;
    const double xp = (bp - apq * xq) / app;
    x0 = pc == 0 ? xp : xq;
    x1 = pc == 0 ? xq : xp;
}

// bilinear face X(xi, eta) = f0 + f1 xi + f2 eta + f3 xi eta
DDPCA_HD void bilinear(const double (&c)[4][3], double (&f)[4][3]) {
    for (int i = 0; i < 3; ++i) {
        f[0][i] = f[1][i] = f[2][i] = f[3][i] = 0.0;
        for (int k = 0; k < 4; ++k) {
            f[0][i] += c[k][i] / 4.0;
            f[1][i] += c[k][i] * corn_x(k) / 4.0;
            f[2][i] += c[k][i] * corn_y(k) / 4.0;
            f[3][i] += c[k][i] * corn_x(k) * corn_y(k) / 4.0;
        }
    }
}

// tangents dX/dxi, dX/deta of a face at (xi, eta)
DDPCA_HD void tangents(const double (&c)[4][3], double xi, double et, double (&t1)[3], double (&t2)[3]) {
    for (int i = 0; i < 3; ++i) {
        t1[i] = t2[i] = 0.0;
        for (int k = 0; k < 4; ++k) {
            t1[i] += c[k][i] * (corn_x(k) / 4.0 + corn_x(k) * corn_y(k) * et / 4.0);
            t2[i] += c[k][i] * (corn_y(k) / 4.0 + corn_x(k) * corn_y(k) * xi / 4.0);
        }
    }
}

// what PROJECT_STM needs of a master face, the same for all four slave corners of a pair
struct Master {
    double f[4][3];
    double f11, f22, f33, f12, f13, f23;
    double diam, cent[3];
};

// the shortest corner distance of a face (PROJECT_STM's step) and its corner mean
DDPCA_HD double face_diam(const double (&c)[4][3], double (&cent)[3]) {
    double diam = 1.0e15;
    cent[0] = cent[1] = cent[2] = 0.0;
    for (int i = 0; i < 4; ++i) {
        for (int j = i + 1; j < 4; ++j) {
            const double e[3] = {c[i][0] - c[j][0], c[i][1] - c[j][1], c[i][2] - c[j][2]};
            diam = dmin(diam, sqrt(dot3(e, e)));
        }
        for (int a = 0; a < 3; ++a) cent[a] += 0.25 * c[i][a];
    }
    return diam;
}

DDPCA_HD void master_face(const double (&c)[4][3], Master& M) {
    bilinear(c, M.f);
    M.f11 = dot3(M.f[1], M.f[1]), M.f22 = dot3(M.f[2], M.f[2]), M.f33 = dot3(M.f[3], M.f[3]);
    M.f12 = dot3(M.f[1], M.f[2]), M.f13 = dot3(M.f[1], M.f[3]), M.f23 = dot3(M.f[2], M.f[3]);
    M.diam = face_diam(c, M.cent);
}

// closest point of P on the master face: Newton on the gradient of |X - P|^2 from (xi, eta)
DDPCA_HD void project_stm_sub(const Master& M, const double (&P)[3], double& xi, double& et) {
    const double d[3] = {M.f[0][0] - P[0], M.f[0][1] - P[1], M.f[0][2] - P[2]};
    const double f11 = M.f11, f22 = M.f22, f33 = M.f33, f12 = M.f12, f13 = M.f13, f23 = M.f23;
    const double d1 = dot3(d, M.f[1]), d2 = dot3(d, M.f[2]), d3 = dot3(d, M.f[3]);
#pragma unroll 1
    for (int it = 0; it < 60; ++it) {
        const double r0 = d1 + f11 * xi + (f12 + d3) * et + 2.0 * f13 * xi * et + f23 * et * et + f33 * xi * et * et;
        const double r1 = d2 + f22 * et + (f12 + d3) * xi + 2.0 * f23 * xi * et + f13 * xi * xi + f33 * xi * xi * et;
        const double j00 = f11 + 2.0 * f13 * et + f33 * et * et;
        const double j01 = (f12 + d3) + 2.0 * f13 * xi + 2.0 * f23 * et + 2.0 * f33 * xi * et;
        const double j10 = (f12 + d3) + 2.0 * f23 * et + 2.0 * f13 * xi + 2.0 * f33 * xi * et;
        const double j11 = f22 + 2.0 * f23 * xi + f33 * xi * xi;
        double dx0, dx1;
        solve2(j00, j01, j10, j11, r0, r1, dx0, dx1);
        dx0 = -dx0;
        dx1 = -dx1;
        if (sqrt(dx0 * dx0 + dx1 * dx1) < 1.0e-12 && sqrt(r0 * r0 + r1 * r1) < 1.0e-15) break;
        xi += dx0;
        et += dx1;
    }
}

// PROJECT_STM: far points are approached in steps of the face's shortest corner distance, at most
// `cap` of them
DDPCA_HD void project_stm(const Master& M, const double (&P)[3], long cap, double& xi, double& et) {
    xi = et = 0.0;
    const double dv[3] = {P[0] - M.cent[0], P[1] - M.cent[1], P[2] - M.cent[2]};
    const double dist = sqrt(dot3(dv, dv));
    const double diam = M.diam;
    if (dist > diam) {
        const double steps = dist / diam;
#pragma unroll 1
        for (long t = 0; t < steps && t < cap; ++t) {
            const double Q[3] = {M.cent[0] + t * diam * dv[0] / dist, M.cent[1] + t * diam * dv[1] / dist,
                                 M.cent[2] + t * diam * dv[2] / dist};
            project_stm_sub(M, Q, xi, et);
        }
    }
    project_stm_sub(M, P, xi, et);
}

// PROJECT_MTS: the slave natural coordinates s of the master point Xm with tangents t1, t2;
// g = bilinear(slave corners)
DDPCA_HD void project_mts(const double (&t1)[3], const double (&t2)[3], const double (&g)[4][3], const double (&Xm)[3],
                          double (&s)[2]) {
    const double e00 = dot3(g[0], t1) - dot3(Xm, t1), e01 = dot3(g[1], t1), e02 = dot3(g[2], t1), e03 = dot3(g[3], t1);
    const double e10 = dot3(g[0], t2) - dot3(Xm, t2), e11 = dot3(g[1], t2), e12 = dot3(g[2], t2), e13 = dot3(g[3], t2);
    s[0] = s[1] = 0.0;
#pragma unroll 1
    for (int it = 0; it < 60; ++it) {
        const double r0 = e00 + e01 * s[0] + e02 * s[1] + e03 * s[0] * s[1];
        const double r1 = e10 + e11 * s[0] + e12 * s[1] + e13 * s[0] * s[1];
        double dx0, dx1;
        solve2(e01 + e03 * s[1], e02 + e03 * s[0], e11 + e13 * s[1], e12 + e13 * s[0], r0, r1, dx0, dx1);
        dx0 = -dx0;
        dx1 = -dx1;
        if (sqrt(dx0 * dx0 + dx1 * dx1) < 1.0e-14 && sqrt(r0 * r0 + r1 * r1) < 1.0e-15) break;
        s[0] += dx0;
        s[1] += dx1;
    }
}

DDPCA_HD double tri_area(double ax, double ay, double bx, double by, double cx, double cy) {
    return fabs((bx - ax) * (cy - ay) - (by - ay) * (cx - ax)) / 2.0;
}

DDPCA_HD void push(const Slots& S, int& n, double x, double y) {
    if (n < kMaxClip) {  // never false: kMaxClip is the bound of what the clip can push
        S.x[n * S.stride] = x;
        S.y[n * S.stride] = y;
        ++n;
    }
}

// segment intersection of p0p1 with p2p3, pushed onto the clip list
DDPCA_HD void segment_cross(double p0x, double p0y, double p1x, double p1y, double p2x, double p2y, double p3x, double p3y,
                            const Slots& S, int& n) {
    if (dmax(p0x, p1x) < dmin(p2x, p3x) || dmax(p0y, p1y) < dmin(p2y, p3y) || dmin(p0x, p1x) > dmax(p2x, p3x) ||
        dmin(p0y, p1y) > dmax(p2y, p3y))
        return;
    const bool straddle =
        ((p2x - p0x) * (p2y - p3y) - (p2y - p0y) * (p2x - p3x)) * ((p2x - p1x) * (p2y - p3y) - (p2y - p1y) * (p2x - p3x)) <= 0 &&
        ((p0x - p2x) * (p0y - p1y) - (p0y - p2y) * (p0x - p1x)) * ((p0x - p3x) * (p0y - p1y) - (p0y - p3y) * (p0x - p1x)) <= 0;
    if (!straddle) return;
    const double a2 = tri_area(p2x, p2y, p0x, p0y, p1x, p1y), a3 = tri_area(p3x, p3y, p0x, p0y, p1x, p1y);
    if (fabs(a2) < kMiniArea && fabs(a3) < kMiniArea) {  // collinear: the overlap
        const bool byx = fabs(p0x - p1x) > 1.0e-10;
        if ((byx ? p0x : p0y) > (byx ? p1x : p1y)) {
            double t = p0x;
            p0x = p1x, p1x = t;
            t = p0y, p0y = p1y, p1y = t;
        }
        if ((byx ? p2x : p2y) > (byx ? p3x : p3y)) {
            double t = p2x;
            p2x = p3x, p3x = t;
            t = p2y, p2y = p3y, p3y = t;
        }
        const bool f2 = (byx ? p0x : p0y) < (byx ? p2x : p2y);
        const bool t3 = (byx ? p1x : p1y) > (byx ? p3x : p3y);
        const double fx = f2 ? p2x : p0x, fy = f2 ? p2y : p0y;
        const double tx = t3 ? p3x : p1x, ty = t3 ? p3y : p1y;
        push(S, n, fx, fy);
        if (!(fabs(fx - tx) < 1.0e-10)) push(S, n, tx, ty);
    } else if (fabs(a2) < kMiniArea) {
        push(S, n, p2x, p2y);
    } else if (fabs(a3) < kMiniArea) {
        push(S, n, p3x, p3y);
    } else {
        const double f = a2 / a3;
        push(S, n, (p2x + f * p3x) / (1.0 + f), (p2y + f * p3y) / (1.0 + f));
    }
}

DDPCA_HD bool in_quad(double px, double py, const double (&qx)[4], const double (&qy)[4]) {
    double s = 0.0;
    for (int i = 0; i < 4; ++i) s += tri_area(px, py, qx[i], qy[i], qx[(i + 1) % 4], qy[(i + 1) % 4]);
    return s <= (1.0 + 1.0e-12) * (tri_area(qx[0], qy[0], qx[1], qy[1], qx[2], qy[2]) +
                                   tri_area(qx[2], qy[2], qx[3], qy[3], qx[0], qy[0]));
}

DDPCA_HD bool xy_less(double ax, double ay, double bx, double by) {
    if (ax < bx - 1.0e-10) return true;
    if (ax <= bx + 1.0e-10) return ay < by - 1.0e-10;
    return false;
}

// The intersection polygon of a master / slave face pair in the master's natural coordinates
// (SI_SUB up to the shoelace): its vertices by angle in S.x / S.y, its centroid in (cx, cy).
// Returns the vertex count, 0 when the pair has no quadrature points.
DDPCA_HD int polygon(const double (&mc)[4][3], const double (&sc)[4][3], long cap, const Slots& S, double& cx, double& cy) {
    const int st = S.stride;
    {
        Master M;
        master_face(mc, M);
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const double P[3] = {i == 0 ? sc[0][0] : i == 1 ? sc[1][0] : i == 2 ? sc[2][0] : sc[3][0],
                                 i == 0 ? sc[0][1] : i == 1 ? sc[1][1] : i == 2 ? sc[2][1] : sc[3][1],
                                 i == 0 ? sc[0][2] : i == 1 ? sc[1][2] : i == 2 ? sc[2][2] : sc[3][2]};
            double xi, et;
            project_stm(M, P, cap, xi, et);
            S.a[i * st] = xi;
            S.a[(4 + i) * st] = et;
        }
    }
    const double mx[4] = {corn_x(0), corn_x(1), corn_x(2), corn_x(3)}, my[4] = {corn_y(0), corn_y(1), corn_y(2), corn_y(3)};
    int n0 = 0;
    {
        const double sx[4] = {S.a[0], S.a[st], S.a[2 * st], S.a[3 * st]};
        const double sy[4] = {S.a[4 * st], S.a[5 * st], S.a[6 * st], S.a[7 * st]};
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            const double px = S.a[i * st], py = S.a[(4 + i) * st];
            if (in_quad(px, py, mx, my)) push(S, n0, px, py);
            if (in_quad(corn_x(i), corn_y(i), sx, sy)) push(S, n0, corn_x(i), corn_y(i));
        }
    }
#pragma unroll 1
    for (int e = 0; e < 16; ++e) {
        const int i = e >> 2, j = e & 3, i1 = (i + 1) & 3, j1 = (j + 1) & 3;
        segment_cross(corn_x(i), corn_y(i), corn_x(i1), corn_y(i1), S.a[j * st], S.a[(4 + j) * st], S.a[j1 * st],
                      S.a[(4 + j1) * st], S, n0);
    }
    if (n0 < 3) return 0;
    // by x then y with 1e-10 slack, stable
#pragma unroll 1
    for (int i = 1; i < n0; ++i) {
        const double vx = S.x[i * st], vy = S.y[i * st];
        int j = i;
        while (j > 0 && xy_less(vx, vy, S.x[(j - 1) * st], S.y[(j - 1) * st])) {
            S.x[j * st] = S.x[(j - 1) * st];
            S.y[j * st] = S.y[(j - 1) * st];
            --j;
        }
        S.x[j * st] = vx;
        S.y[j * st] = vy;
    }
    // de-duplicate against the sorted predecessor, in place
    int n = 1;
    double qx = S.x[0], qy = S.y[0];
    double cmx = qx, cmy = qy;
#pragma unroll 1
    for (int i = 1; i < n0; ++i) {
        const double vx = S.x[i * st], vy = S.y[i * st];
        if (fabs(vx - qx) > 1.0e-10 || fabs(vy - qy) > 1.0e-10) {
            S.x[n * st] = vx;
            S.y[n * st] = vy;
            cmx += vx, cmy += vy;
            ++n;
        }
        qx = vx, qy = vy;
    }
    cmx /= (double)n;
    cmy /= (double)n;
    // by angle about the vertex mean
#pragma unroll 1
    for (int i = 0; i < n; ++i) S.a[i * st] = atan2(S.y[i * st] - cmy, S.x[i * st] - cmx);
#pragma unroll 1
    for (int i = 1; i < n; ++i) {
        const double vx = S.x[i * st], vy = S.y[i * st], va = S.a[i * st];
        int j = i;
        while (j > 0 && va < S.a[(j - 1) * st]) {
            S.x[j * st] = S.x[(j - 1) * st];
            S.y[j * st] = S.y[(j - 1) * st];
            S.a[j * st] = S.a[(j - 1) * st];
            --j;
        }
        S.x[j * st] = vx;
        S.y[j * st] = vy;
        S.a[j * st] = va;
    }
    // area and centroid (shoelace)
    double area = 0.0;
    cx = cy = 0.0;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        const int i1 = i + 1 == n ? 0 : i + 1;
        const double ax = S.x[i * st], ay = S.y[i * st], bx = S.x[i1 * st], by = S.y[i1 * st];
        const double cr = ax * by - bx * ay;
        area += cr;
        cx += (ax + bx) * cr;
        cy += (ay + by) * cr;
    }
    area /= 2.0;
    if (fabs(area) <= kMiniArea) return 0;
    cx = cx / 6.0 / area;
    cy = cy / 6.0 / area;
    return n;
}

// quadrature point q (0 .. 4 n - 1) of the polygon: TRIANGLE_QUADRATURE on (centroid, v_t, v_t+1),
// t = q / 4, the 4-point collapsed Gauss rule
DDPCA_HD void quad_point(const Slots& S, int n, double cx, double cy, int q, double& px, double& py, double& wq) {
    const int t = q >> 2, i = (q >> 1) & 1, j = q & 1, t1 = t + 1 == n ? 0 : t + 1;
    const double v1x = S.x[t * S.stride], v1y = S.y[t * S.stride], v2x = S.x[t1 * S.stride], v2y = S.y[t1 * S.stride];
    const double a = tri_area(cx, cy, v1x, v1y, v2x, v2y);
    const double g = sqrt(1.0 / 3.0);
    const double gi = i == 0 ? -g : g, gj = j == 0 ? -g : g;
    const double b0 = (1.0 + gi) / 2.0, b1 = (1.0 - gi) * (1.0 + gj) / 4.0, b2 = 1.0 - b0 - b1;
    px = b0 * cx + b1 * v1x + b2 * v2x;
    py = b0 * cy + b1 * v1y + b2 * v2y;
    wq = 2.0 * a * ((1.0 - gi) / 8.0);
}

// one integration point (SEGMENT_INTERSECT's point assembly): master point (px, py) with polygon
// weight wq; g = bilinear(slave corners)
struct Point {
    double shap[2][4];
    double basis[3][3];
    double gap, w;
};
DDPCA_HD void point(const double (&mc)[4][3], const double (&sc)[4][3], const double (&g)[4][3], double px, double py,
                    double wq, Point& p) {
    double Xm[3] = {0.0, 0.0, 0.0}, Xs[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 4; ++k) {
        p.shap[0][k] = (1.0 + corn_x(k) * px) * (1.0 + corn_y(k) * py) / 4.0;
        for (int a = 0; a < 3; ++a) Xm[a] += p.shap[0][k] * mc[k][a];
    }
    double t1[3], t2[3], s[2];
    tangents(mc, px, py, t1, t2);
    project_mts(t1, t2, g, Xm, s);
    double tc[3], nrm[3], e1[3], e2[3];
    cross3(t1, t2, tc);
    normalized(tc, nrm);
    normalized(t1, e1);
    normalized(t2, e2);
    const double wf = sqrt(tc[0] * tc[0] + tc[1] * tc[1] + tc[2] * tc[2]);
    for (int k = 0; k < 4; ++k) {
        p.shap[1][k] = (1.0 + corn_x(k) * s[0]) * (1.0 + corn_y(k) * s[1]) / 4.0;
        for (int a = 0; a < 3; ++a) Xs[a] += p.shap[1][k] * sc[k][a];
    }
    for (int a = 0; a < 3; ++a) {
        p.basis[0][a] = nrm[a];
        p.basis[1][a] = e1[a];
        p.basis[2][a] = e2[a];
    }
    p.gap = (Xs[0] - Xm[0]) * nrm[0] + (Xs[1] - Xm[1]) * nrm[1] + (Xs[2] - Xm[2]) * nrm[2];
    p.w = wq * wf;
}

// The pair's point count under CONTACT_SEARCH's keep rule: 4 n when one of its points has
// gap <= maxiDist, else 0.  Leaves the polygon in S and its centroid in (cx, cy).
DDPCA_HD int pair_count(const double (&mc)[4][3], const double (&sc)[4][3], long cap, double maxiDist, const Slots& S,
                        double& cx, double& cy) {
    const int n = polygon(mc, sc, cap, S, cx, cy);
    if (n == 0) return 0;
    double g[4][3];
    bilinear(sc, g);
#pragma unroll 1
    for (int q = 0; q < 4 * n; ++q) {
        double px, py, wq;
        quad_point(S, n, cx, cy, q, px, py, wq);
        Point p;
        point(mc, sc, g, px, py, wq, p);
        if (p.gap <= maxiDist) return 4 * n;
    }
    return 0;
}

}  // namespace csface
}  // namespace ddpca
