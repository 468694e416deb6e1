// Dense setup inverses on rocSOLVER / rocBLAS (setup only): the SPD inverse (potrf + potri), the
// LU inverse (getrf + getri), checked or not, and the SVD pseudo-inverse, each in place on an
// n x n device matrix.  A row-major buffer read column-major is the transpose, whose inverse read
// back row-major is the inverse: the forms below hold for either reading.  The caller takes
// solver_lock() (device_common.hpp) around the handle's life where it must.
#pragma once
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>

#include <cstdint>
#include <vector>

#include "../../include/ddpca_amd.h"
#include "device_common.hpp"

namespace ddpca {

// A rocBLAS handle on `stream` for the length of a scope (destroyed on a throw out of it too).
struct BlasHandle {
    rocblas_handle h = nullptr;
    hipStream_t stream = nullptr;
    explicit BlasHandle(hipStream_t st);
    ~BlasHandle();
    BlasHandle(const BlasHandle&) = delete;
    BlasHandle& operator=(const BlasHandle&) = delete;
};

// ---- in place on a device pointer
// Enqueue potrf + potri (lower, on the column-major view) and the mirror of the computed triangle
// into the other one.  info: two zeroed device ints (potrf's, potri's), read by the caller once
// the stream is synchronised.  False: rocSOLVER refused a call.
bool spd_inverse_device(const BlasHandle& h, double* A, int64_t n, rocblas_int* info);
// Enqueue getrf + getri with no check of the pivots; ipiv: n device ints, info as above.
bool lu_inverse_device(const BlasHandle& h, double* A, int64_t n, rocblas_int* ipiv, rocblas_int* info);
// getrf + getri when the LU is clearly regular (every |U_ii| above 1e-10 of the largest) and the
// inverse checks out (||A^-1 A - I||_inf <= 1e-6 by a rocBLAS gemm against a kept copy of A);
// returns false, A overwritten, otherwise, and *resid the residual it measured (INFINITY when the
// pivot test failed).  Synchronises the stream.
bool inv_general_lu_device(const BlasHandle& h, double* A, int64_t n, double* resid);
// Pseudo-inverse by gesvd, singular values below 1e-11 of the largest dropped (*dropped counts
// them).  Synchronises the stream; throws when gesvd fails.
void pinv_general_device(const BlasHandle& h, double* A, int64_t n, int64_t* dropped);

// ---- the same on a host matrix (upload, the form above under solver_lock(), download)
void invert_spd_device(std::vector<double>& A, int64_t n, hipStream_t st);  // throws when not positive definite
bool inv_general_lu_device(std::vector<double>& A, int64_t n, hipStream_t st, double* resid);  // false: A untouched
void pinv_general_device(std::vector<double>& A, int64_t n, hipStream_t st, int64_t* dropped);

}  // namespace ddpca
