// Element arithmetic of STRESS_RECOVERY (MULTIGRID.h:1338-1372) shared by the host restatement
// (stress.cpp) and the device kernels (device_stress.hip), so that both run the same operations in
// the same order.  Plain inline functions: nothing here names a device symbol.
//
// The trilinear map is kept in modal form, x(xi, eta, zeta) = c0 + c1 xi + c2 eta + c3 zeta +
// c4 xi eta + c5 eta zeta + c6 zeta xi + c7 xi eta zeta with c_i = 1/8 sum_k s_i(k) X_k, and the
// displacement likewise.  The Jacobian J = dN X and the reference-space displacement gradient
// G = dN U are then 27 multiply-adds each per Gauss point instead of 72, and
// sigma_g = D B u_e becomes D applied to the strain of grad u = J^-1 G (the same product, summed
// over the corners first).
#pragma once

#if defined(__HIPCC__)
#define DDPCA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DDPCA_HD inline
#endif

namespace ddpca {
namespace stress {

// corner k of the reference hex (PREP.h, the order of MULTIGRID::elemVect[].cornNode)
DDPCA_HD double sgn_xi(int k) { return (k == 1 || k == 2 || k == 5 || k == 6) ? 1.0 : -1.0; }
DDPCA_HD double sgn_eta(int k) { return (k == 2 || k == 3 || k == 6 || k == 7) ? 1.0 : -1.0; }
DDPCA_HD double sgn_zeta(int k) { return k >= 4 ? 1.0 : -1.0; }
// s_i(k): the sign of corner k in mode i (1, xi, eta, zeta, xi eta, eta zeta, zeta xi, xi eta zeta)
DDPCA_HD double mode_sign(int i, int k) {
    const double a = sgn_xi(k), b = sgn_eta(k), c = sgn_zeta(k);
    return i == 0 ? 1.0 : i == 1 ? a : i == 2 ? b : i == 3 ? c : i == 4 ? a * b : i == 5 ? b * c : i == 6 ? c * a : a * b * c;
}

// 3-point Gauss rule (PREP.h:235-281): g = i * 9 + j * 3 + k over (xi, eta, zeta)
DDPCA_HD double gauss_pt(int i) { return i == 0 ? -0.7745966692414834 : i == 1 ? 0.0 : 0.7745966692414834; }
DDPCA_HD double gauss_wt(int i) { return i == 1 ? 8.0 / 9.0 : 5.0 / 9.0; }

// N_k at (x, y, z)
DDPCA_HD double shape(double sx, double sy, double sz, double x, double y, double z) {
    return (1.0 + sx * x) * (1.0 + sy * y) * (1.0 + sz * z) * 0.125;
}

// det J and the Voigt stress (xx, yy, zz, xy, yz, zx) at one Gauss point from the modal
// coefficients of the geometry (C) and of the displacement (U)
DDPCA_HD double gauss_stress(const double (&C)[8][3], const double (&U)[8][3], double x, double y, double z, double lam,
                             double mu, double (&sig)[6]) {
    const double yz = y * z, xz = x * z, xy = x * y;
    double J[3][3], G[3][3];
    for (int c = 0; c < 3; ++c) {
        J[0][c] = C[1][c] + C[4][c] * y + C[6][c] * z + C[7][c] * yz;
        J[1][c] = C[2][c] + C[4][c] * x + C[5][c] * z + C[7][c] * xz;
        J[2][c] = C[3][c] + C[5][c] * y + C[6][c] * x + C[7][c] * xy;
        G[0][c] = U[1][c] + U[4][c] * y + U[6][c] * z + U[7][c] * yz;
        G[1][c] = U[2][c] + U[4][c] * x + U[5][c] * z + U[7][c] * xz;
        G[2][c] = U[3][c] + U[5][c] * y + U[6][c] * x + U[7][c] * xy;
    }
    const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                       J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
    const double r = 1.0 / det;
    double Ji[3][3];
    Ji[0][0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) * r;
    Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * r;
    Ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * r;
    Ji[1][0] = (J[1][2] * J[2][0] - J[1][0] * J[2][2]) * r;
    Ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * r;
    Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * r;
    Ji[2][0] = (J[1][0] * J[2][1] - J[1][1] * J[2][0]) * r;
    Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * r;
    Ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * r;
    // grad[a][c] = d u_a / d x_c = sum_r Ji[c][r] G[r][a]
    double grad[3][3];
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) grad[a][c] = Ji[c][0] * G[0][a] + Ji[c][1] * G[1][a] + Ji[c][2] * G[2][a];
    const double tr = lam * (grad[0][0] + grad[1][1] + grad[2][2]);
    sig[0] = tr + 2.0 * mu * grad[0][0];
    sig[1] = tr + 2.0 * mu * grad[1][1];
    sig[2] = tr + 2.0 * mu * grad[2][2];
    sig[3] = mu * (grad[0][1] + grad[1][0]);
    sig[4] = mu * (grad[1][2] + grad[2][1]);
    sig[5] = mu * (grad[2][0] + grad[0][2]);
    return det;
}

// the mean of the rows of one element's nodal stresses (48 doubles, row-major 8 x 6) that `mask`
// selects, corners ascending
DDPCA_HD void masked_mean(const double* se, unsigned mask, double (&out)[6]) {
    for (int c = 0; c < 6; ++c) out[c] = 0.0;
    int n = 0;
    for (int k = 0; k < 8; ++k)
        if (mask >> k & 1u) {
            for (int c = 0; c < 6; ++c) out[c] += se[6 * k + c];
            ++n;
        }
    if (n > 1)
        for (int c = 0; c < 6; ++c) out[c] /= (double)n;
}

DDPCA_HD double von_mises_sq(const double (&s)[6]) {
    const double a = s[0] - s[1], b = s[1] - s[2], c = s[0] - s[2];
    return (a * a + b * b + c * c + 6.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5])) / 2.0;
}

}  // namespace stress
}  // namespace ddpca
