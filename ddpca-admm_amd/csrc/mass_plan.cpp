// Host-side setup of the batched surface-mass solver: see mass_plan.hpp.
#include "mass_plan.hpp"

#include <algorithm>
#include <cmath>

namespace ddpca {

void mass_spectrum(const Csr& M, int m, double* lmin, double* lmax, double* gersh) {
    const int64_t n = M.nrow;
    std::vector<double> dis(n, 0.0);
    double g = 0.0;
    for (int64_t r = 0; r < n; ++r) {
        double dg = 0.0, sa = 0.0;
        for (int64_t k = M.ptr[r]; k < M.ptr[r + 1]; ++k) {
            sa += std::abs(M.val[k]);
            if (M.col[k] == r) dg = M.val[k];
        }
        dis[r] = dg > 0.0 ? 1.0 / std::sqrt(dg) : 0.0;
        if (dg > 0.0) g = std::max(g, sa / dg);
    }
    *gersh = g;
    m = (int)std::min<int64_t>(m, n);
    std::vector<double> v(n), vp(n, 0.0), w(n), alpha, beta;
    double nv = 0.0;
    for (int64_t i = 0; i < n; ++i) v[i] = 1.0 + 0.5 * std::sin(0.7 * (double)i + 0.3), nv += v[i] * v[i];
    nv = std::sqrt(nv);
    for (double& x : v) x /= nv;
    double bprev = 0.0;
    for (int j = 0; j < m; ++j) {
        for (int64_t r = 0; r < n; ++r) {
            double acc = 0.0;
            for (int64_t k = M.ptr[r]; k < M.ptr[r + 1]; ++k) acc += M.val[k] * dis[M.col[k]] * v[M.col[k]];
            w[r] = dis[r] * acc - bprev * vp[r];
        }
        double a = 0.0;
        for (int64_t r = 0; r < n; ++r) a += w[r] * v[r];
        double b = 0.0;
        for (int64_t r = 0; r < n; ++r) {
            w[r] -= a * v[r];
            b += w[r] * w[r];
        }
        b = std::sqrt(b);
        alpha.push_back(a);
        if (j + 1 == m || !(b > 1e-14)) break;
        beta.push_back(b);
        for (int64_t r = 0; r < n; ++r) {
            vp[r] = v[r];
            v[r] = w[r] / b;
        }
        bprev = b;
    }
    const int t = (int)alpha.size();
    auto count_below = [&](double x) {  // eigenvalues of T below x (Sturm sequence)
        int c = 0;
        double q = alpha[0] - x;
        if (q < 0) ++c;
        for (int i = 1; i < t; ++i) {
            const double qq = std::abs(q) < 1e-300 ? 1e-300 : q;
            q = alpha[i] - x - beta[i - 1] * beta[i - 1] / qq;
            if (q < 0) ++c;
        }
        return c;
    };
    double lo = 0.0, hi = 0.0;
    for (int i = 0; i < t; ++i) {
        const double rad = (i > 0 ? std::abs(beta[i - 1]) : 0.0) + (i + 1 < t ? std::abs(beta[i]) : 0.0);
        lo = std::min(lo, alpha[i] - rad);
        hi = std::max(hi, alpha[i] + rad);
    }
    auto kth = [&](int k) {  // the k-th smallest eigenvalue (0-based)
        double a = lo, b = hi;
        for (int it = 0; it < 200; ++it) {
            const double mid = 0.5 * (a + b);
            if (count_below(mid) > k) b = mid;
            else a = mid;
        }
        return 0.5 * (a + b);
    };
    *lmin = kth(0);
    *lmax = kth(t - 1);
}

MassPlan mass_plan(const std::vector<const Csr*>& A, const std::vector<int64_t>& roff, int64_t nrow, bool cheb) {
    MassPlan P;
    const int nsys = (int)A.size();
    const int64_t nch = P.nch = nrow / 64;
    auto pad64 = [](int64_t n) { return (n + 63) / 64 * 64; };
    auto &sl = P.slots, &cs = P.csys, &co = P.col;
    auto &of = P.off, &c0 = P.cb;
    auto &va = P.val, &di = P.dinv;
    sl.assign(std::max<int64_t>(nch, 1), 0);
    cs.assign(std::max<int64_t>(nch, 1), 0);
    of.assign(nch + 1, 0);
    c0.assign(nsys + 1, nch);
    di.assign(std::max<int64_t>(nrow, 1), 0.0);
    for (int s = 0; s < nsys; ++s) {
        const Csr& M = *A[s];
        c0[s] = roff[s] / 64;
        for (int64_t c = roff[s] / 64; c < (roff[s] + pad64(M.nrow)) / 64; ++c) {
            cs[c] = s;
            int64_t mx = 0;
            for (int64_t r = (c * 64 - roff[s]); r < std::min(M.nrow, c * 64 - roff[s] + 64); ++r)
                mx = std::max(mx, M.ptr[r + 1] - M.ptr[r]);
            sl[c] = (int32_t)mx;
        }
    }
    for (int64_t c = 0; c < nch; ++c) of[c + 1] = of[c] + sl[c];
    co.assign(std::max<int64_t>(of[nch] * 64, 1), 0);
    va.assign(std::max<int64_t>(of[nch] * 64, 1), 0.0);
    for (int64_t c = 0; c < nch; ++c)
        for (int64_t q2 = of[c]; q2 < of[c + 1]; ++q2)
            for (int lane = 0; lane < 64; ++lane) co[q2 * 64 + lane] = (int32_t)(c * 64 + lane);  // pad: self, 0
    for (int s = 0; s < nsys; ++s) {
        const Csr& M = *A[s];
        for (int64_t r0 = 0; r0 < M.nrow; ++r0) {
            const int64_t g = roff[s] + r0, c = g / 64, lane = g % 64;
            for (int64_t k2 = M.ptr[r0]; k2 < M.ptr[r0 + 1]; ++k2) {
                const int64_t q2 = of[c] + (k2 - M.ptr[r0]);
                co[q2 * 64 + lane] = (int32_t)(roff[s] + M.col[k2]);
                va[q2 * 64 + lane] = M.val[k2];
                if (M.col[k2] == r0) di[g] = 1.0 / M.val[k2];
            }
        }
    }
    // paired batch: systems i and i + nsys/2 share one matrix, R = nrow/2 rows apart
    P.paired = nsys >= 2 && nsys % 2 == 0 && nrow % 128 == 0;
    for (int s = 0; P.paired && s < nsys / 2; ++s)
        P.paired = A[s] == A[s + nsys / 2] && roff[s + nsys / 2] == roff[s] + nrow / 2;
    P.cheb = cheb && nsys > 0;
    P.lam_lo.assign(nsys, 0.0);
    P.lam_hi.assign(nsys, 0.0);
    if (P.cheb) {
        std::vector<double> lo(nsys), hi(nsys), gh(nsys);
#pragma omp parallel for schedule(dynamic, 1)
        for (int s2 = 0; s2 < nsys; ++s2) mass_spectrum(*A[s2], 60, &lo[s2], &hi[s2], &gh[s2]);
        for (int s2 = 0; s2 < nsys; ++s2) {
            P.lam_lo[s2] = 0.9 * lo[s2];
            P.lam_hi[s2] = std::min(gh[s2], 1.05 * hi[s2]);
            if (!(P.lam_lo[s2] > 0.0) || !(P.lam_hi[s2] > P.lam_lo[s2])) P.cheb = false;
        }
    }
    return P;
}

ChebPlan cheb_plan(const std::vector<double>& lam_lo, const std::vector<double>& lam_hi, double rtol) {
    ChebPlan C;
    const int nsys = (int)lam_lo.size();
    C.ks.assign(nsys, 0);
    int64_t K = 0;
    for (int s2 = 0; s2 < nsys; ++s2) {
        const double kap = lam_hi[s2] / lam_lo[s2], sk = std::sqrt(kap);
        const double sig = (sk + 1.0) / (sk - 1.0);
        const int64_t ks = (int64_t)std::ceil(std::log(4.0 * sk / rtol) / std::log(sig));
        C.ks[s2] = (int32_t)std::max<int64_t>(1, ks);
        K = std::max<int64_t>(K, C.ks[s2]);
    }
    C.K = K;
    if (K > kChebMax) return C;
    C.coef.assign((size_t)2 * K * nsys, 0.0);
    C.ith.resize(nsys);
    for (int s2 = 0; s2 < nsys; ++s2) {
        const double th = 0.5 * (lam_hi[s2] + lam_lo[s2]), de = 0.5 * (lam_hi[s2] - lam_lo[s2]);
        const double s1 = th / de;
        C.ith[s2] = 1.0 / th;
        double rho = 1.0 / s1;
        for (int64_t kk = 0; kk < K; ++kk) {
            const double rn = 1.0 / (2.0 * s1 - rho);
            C.coef[2 * (kk * nsys + s2)] = rn * rho;
            C.coef[2 * (kk * nsys + s2) + 1] = 2.0 * rn / de;
            rho = rn;
        }
    }
    return C;
}

}  // namespace ddpca
