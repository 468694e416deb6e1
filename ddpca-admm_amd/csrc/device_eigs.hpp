// Device eigen-solver: the nev eigenpairs of smallest magnitude of a symmetric positive definite
// operator A from thick-restart Lanczos on A^-1 (device_eigs.hip).  The driver owns no solver
// state of its caller: A^-1 is an "apply to column j, write column j + 1" callback and A itself a
// device CSR used for the true residual only.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "device_common.hpp"

namespace ddpca {

constexpr int kEigsMaxNcv = 512;  // basis columns the kernels' LDS tables and the host solve hold

// fp64 CSR of A on the device (n x n, both triangles)
struct EigsCsr {
    const int64_t* ptr = nullptr;
    const int32_t* col = nullptr;
    const double* val = nullptr;
};

// y = A^-1 x, enqueued on (or joined to) the driver's stream; x and y are columns of the basis
using EigsApply = std::function<void(const double* x, double* y)>;

struct EigsResult {
    std::vector<double> theta, resid;  // nev each, theta ascending; resid = ||A y - theta y|| / theta
    int64_t steps = 0, restarts = 0, applies = 0;
    bool converged = false;
    // HIP-event times in ms when timed: operator applications, orthogonalisation (start vector
    // included), Ritz products (Y = V S, A Y, the restart's compression)
    double ms[3] = {0.0, 0.0, 0.0};
};

// Thick-restart Lanczos with full reorthogonalisation (classical Gram-Schmidt, twice) on A^-1.
// Y: device, n x nev column-major, gets the Ritz vectors of the last convergence check (unit
// norm, column k belongs to theta[k]).  Returns with converged = false after max_restarts restarts
// (the best pairs filled in); never loops on.  Requires 1 <= nev < ncv <= min(n, kEigsMaxNcv).
void eigs_smallest(hipStream_t st, int64_t n, const EigsApply& apply_inv, const EigsCsr& A, int nev, int ncv, double tol,
                   int64_t max_restarts, bool timed, double* Y, EigsResult& out);

// Host: eigen-decomposition of the symmetric m x m matrix a (row-major, destroyed) by cyclic
// Jacobi rotations.  w ascending; z row-major m x m, column q the eigenvector of w[q].
void sym_eig_jacobi(int m, std::vector<double>& a, std::vector<double>& w, std::vector<double>& z);

// Measurement (profiles/apps_probe.py): ms per launch pair of one Gram-Schmidt pass of an n-vector
// against m columns, out[0] the kernels of this file (k_eig_vtw + k_eig_vtw_fin, k_eig_update),
// out[1] the same pass composed from device_krylov.hip's k_mdot / k_vcomb (krylov_cgs_pass).
void eigs_orth_bench(int device, int64_t n, int m, int reps, double out[4]);
// the composed pass: c = V^T w by k_mdot (kMaxDots columns per launch) + k_mdot_fin, then
// w -= V c by k_vcomb (kMaxBasis columns per launch); scratch: partial (12 x 1024), cdev (m)
void krylov_cgs_pass(hipStream_t st, int64_t n, const double* V, int64_t ld, int m, double* w, double* partial, double* cdev,
                     double* chost);

}  // namespace ddpca
