// Host-side setup of the batched surface-mass solver (MassBatch, device_mass.hpp): what is derived
// from the systems before anything reaches the device -- the ELL-64 packing, the pair detection,
// the spectrum bounds and the Chebyshev step counts and coefficients.  Plain C++ (no HIP), so the
// host sanitizer build covers it (tests/sanitize).
#pragma once
#include <cstdint>
#include <vector>

#include "sparse.hpp"

namespace ddpca {

constexpr int64_t kChebMax = 120;  // Chebyshev steps per solve; a plan past it runs the plain CG

// Rows of all systems concatenated, each padded to a multiple of 64 (ELL-64: chunk = 64 rows = one
// wave, lane = row, slot k at (off[c] + k) * 64 + lane).
struct MassPlan {
    int64_t nch = 0;
    std::vector<int32_t> slots, csys;  // per chunk: stored slots, system
    std::vector<int64_t> off, cb;      // first slot of chunk c (nch + 1); first chunk of system s (nsys + 1)
    std::vector<int32_t> col;          // padding slots: the row itself, value 0
    std::vector<double> val, dinv;
    bool paired = false;               // systems i and i + nsys/2 share one matrix, nrow/2 rows apart
    bool cheb = false;                 // every system has usable bounds
    std::vector<double> lam_lo, lam_hi;  // D^-1 M spectrum bounds used, per system (cheb)
};

// A[i] = system i (rows m_i), placed at rows roff[i] (multiples of 64) of nrow_total; cheb: also
// the Chebyshev bounds [0.9 Ritz min, min(Gershgorin, 1.05 Ritz max)] of D^-1 M after 60 Lanczos
// steps (the CG that follows the fixed step count repairs an estimate that was off)
MassPlan mass_plan(const std::vector<const Csr*>& A, const std::vector<int64_t>& roff, int64_t nrow_total, bool cheb);

// Extreme eigenvalues of D^-1 M for an SPD CSR M: Lanczos on the symmetric D^-1/2 M D^-1/2 (m steps
// from a fixed start vector), Ritz extremes by bisection on the tridiagonal (Sturm counts);
// *gersh = max_i sum_j |M_ij| / M_ii, an upper bound
void mass_spectrum(const Csr& M, int m, double* lmin, double* lmax, double* gersh);

// The step counts and coefficients for a relative residual rtol: per system kappa = hi / lo,
// K = ceil(ln(4 sqrt(kappa) / rtol) / ln sigma), sigma = (sqrt(kappa) + 1) / (sqrt(kappa) - 1)
// (the residual bound 2 sqrt(kappa) sigma^-K at half of rtol).  coef[(k nsys + s) 2 + {0, 1}] and
// ith[s] = 1 / theta_s are filled only while K = max ks <= kChebMax.
struct ChebPlan {
    int64_t K = 0;
    std::vector<int32_t> ks;
    std::vector<double> coef, ith;
};
ChebPlan cheb_plan(const std::vector<double>& lam_lo, const std::vector<double>& lam_hi, double rtol);

}  // namespace ddpca
