// Dense setup inverses on rocSOLVER / rocBLAS (device_dense.hpp): MgpisDevice's exact coarse
// solves and MCONTACT's coarse space.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include "device_dense.hpp"

namespace ddpca {

namespace {
// potri(lower) on the column-major view leaves the inverse in the row-major upper triangle;
// mirror it into the lower one
__global__ void k_mirror_upper(double* A, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n) return;
    const int64_t i = idx / n, j = idx % n;
    if (j < i) A[i * n + j] = A[j * n + i];
}

// Scale row i of the column-major n x n matrix Vt by 1 / s_i, or 0 when s_i <= tol (pseudo-inverse)
__global__ void k_pinv_rows(double* Vt, const double* S, int64_t n, double tol) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n) return;
    const double sv = S[idx % n];
    Vt[idx] *= sv > tol ? 1.0 / sv : 0.0;
}

__global__ void k_diag(const double* A, int64_t n, double* d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = A[i * n + i];
}

// row sums of |M - I| (M column-major n x n): the residual of an inverse read as M = A^-1 A
__global__ void k_resid_rows(const double* M, int64_t n, double* r) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s += std::abs(M[i * n + j] - (i == j ? 1.0 : 0.0));
    r[j] = s;
}

constexpr double kLuMaxResid = 1e-6;
}  // namespace

BlasHandle::BlasHandle(hipStream_t st) : stream(st) {
    if (rocblas_create_handle(&h) != rocblas_status_success) throw ApiError(DDPCA_EHIP, "rocblas_create_handle");
    rocblas_set_stream(h, st);
}

BlasHandle::~BlasHandle() { rocblas_destroy_handle(h); }

bool spd_inverse_device(const BlasHandle& h, double* A, int64_t n, rocblas_int* info) {
    const rocblas_status s1 = rocsolver_dpotrf(h.h, rocblas_fill_lower, (rocblas_int)n, A, (rocblas_int)n, info);
    const rocblas_status s2 = rocsolver_dpotri(h.h, rocblas_fill_lower, (rocblas_int)n, A, (rocblas_int)n, info + 1);
    hipLaunchKernelGGL(k_mirror_upper, dim3(std::max<int64_t>(1, (n * n + 255) / 256)), dim3(256), 0, h.stream, A, n);
    return s1 == rocblas_status_success && s2 == rocblas_status_success;
}

bool lu_inverse_device(const BlasHandle& h, double* A, int64_t n, rocblas_int* ipiv, rocblas_int* info) {
    const rocblas_status s1 = rocsolver_dgetrf(h.h, (rocblas_int)n, (rocblas_int)n, A, (rocblas_int)n, ipiv, info);
    const rocblas_status s2 = rocsolver_dgetri(h.h, (rocblas_int)n, A, (rocblas_int)n, ipiv, info + 1);
    return s1 == rocblas_status_success && s2 == rocblas_status_success;
}

// (LAGRANGE's condensed coarse operators, 4851 rows at BLOCK: ~20 s per Newton step by gesvd.)
bool inv_general_lu_device(const BlasHandle& h, double* A, int64_t n, double* resid) {
    *resid = INFINITY;
    hipStream_t st = h.stream;
    DevBuf<double> a0(std::max<int64_t>(n * n, 1)), diag(std::max<int64_t>(n, 1));
    DDPCA_HIP(hipMemcpyAsync(a0.p, A, n * n * sizeof(double), hipMemcpyDeviceToDevice, st));
    DevBuf<rocblas_int> ipiv(std::max<int64_t>(n, 1)), info(2);
    info.zero(st);
    const rocblas_status s1 = rocsolver_dgetrf(h.h, (rocblas_int)n, (rocblas_int)n, A, (rocblas_int)n, ipiv.p, info.p);
    hipLaunchKernelGGL(k_diag, dim3(std::max<int64_t>(1, (n + 255) / 256)), dim3(256), 0, st, A, n, diag.p);
    DDPCA_HIP(hipStreamSynchronize(st));
    const auto u = diag.download();
    double umax = 0.0, umin = INFINITY;
    for (double x : u) {
        umax = std::max(umax, std::abs(x));
        umin = std::min(umin, std::abs(x));
    }
    if (s1 != rocblas_status_success || info.download()[0] != 0 || !(umin > 1e-10 * umax)) return false;
    const rocblas_status s2 = rocsolver_dgetri(h.h, (rocblas_int)n, A, (rocblas_int)n, ipiv.p, info.p + 1);
    // column-major: A = (A0^T)^-1 and a0 = A0^T, so M = A a0 = (A0 A0^-1)^T; ||M - I|| by column sums
    // of M (= row sums of A0 A0^-1 - I)
    DevBuf<double> M(std::max<int64_t>(n * n, 1)), rs(std::max<int64_t>(n, 1));
    const double one = 1.0, zero = 0.0;
    const rocblas_status s3 = rocblas_dgemm(h.h, rocblas_operation_none, rocblas_operation_none, (rocblas_int)n, (rocblas_int)n,
                                            (rocblas_int)n, &one, A, (rocblas_int)n, a0.p, (rocblas_int)n, &zero, M.p,
                                            (rocblas_int)n);
    hipLaunchKernelGGL(k_resid_rows, dim3(std::max<int64_t>(1, (n + 255) / 256)), dim3(256), 0, st, M.p, n, rs.p);
    DDPCA_HIP(hipStreamSynchronize(st));
    if (s2 != rocblas_status_success || s3 != rocblas_status_success || info.download()[1] != 0) return false;
    double r = 0.0;
    for (double x : rs.download()) r = std::max(r, x);
    *resid = r;
    return r <= kLuMaxResid;
}

// rocSOLVER gesvd of the buffer read column-major (M = A^T = U S Vt), then C = Vt^T S+ U^T (rocBLAS
// gemm) = (A^+)^T column-major, i.e. A^+ row-major.  The coarse operator of LAGRANGE's condensed
// system is singular when a frictionless contact leaves a body free to slide (the reference's LDLT
// meets the same zero pivots); the V-cycle then solves on the range.
void pinv_general_device(const BlasHandle& h, double* A, int64_t n, int64_t* dropped) {
    hipStream_t st = h.stream;
    DevBuf<double> S(std::max<int64_t>(n, 1)), U(std::max<int64_t>(n * n, 1)), Vt(std::max<int64_t>(n * n, 1)),
        E(std::max<int64_t>(n, 1)), C(std::max<int64_t>(n * n, 1));
    DevBuf<rocblas_int> info(1);
    info.zero(st);
    const rocblas_status s1 = rocsolver_dgesvd(h.h, rocblas_svect_all, rocblas_svect_all, (rocblas_int)n, (rocblas_int)n, A,
                                               (rocblas_int)n, S.p, U.p, (rocblas_int)n, Vt.p, (rocblas_int)n, E.p,
                                               rocblas_outofplace, info.p);
    std::vector<double> sv(n);
    DDPCA_HIP(hipMemcpyAsync(sv.data(), S.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    DDPCA_HIP(hipStreamSynchronize(st));
    if (s1 != rocblas_status_success || info.download()[0] != 0)
        throw ApiError(DDPCA_EHIP, "rocsolver gesvd failed on the coarse operator");
    const double tol = 1e-11 * (n ? sv[0] : 0.0);
    *dropped = 0;
    for (double x : sv) *dropped += !(x > tol);
    hipLaunchKernelGGL(k_pinv_rows, dim3(std::max<int64_t>(1, (n * n + 255) / 256)), dim3(256), 0, st, Vt.p, S.p, n, tol);
    const double one = 1.0, zero = 0.0;
    const rocblas_status s2 = rocblas_dgemm(h.h, rocblas_operation_transpose, rocblas_operation_transpose, (rocblas_int)n,
                                            (rocblas_int)n, (rocblas_int)n, &one, Vt.p, (rocblas_int)n, U.p, (rocblas_int)n,
                                            &zero, C.p, (rocblas_int)n);
    DDPCA_HIP(hipMemcpyAsync(A, C.p, n * n * sizeof(double), hipMemcpyDeviceToDevice, st));
    DDPCA_HIP(hipStreamSynchronize(st));
    if (s2 != rocblas_status_success) throw ApiError(DDPCA_EHIP, "rocblas gemm failed");
}

// ---- host-matrix forms
void invert_spd_device(std::vector<double>& A, int64_t n, hipStream_t st) {
    DevBuf<double> d;
    d.upload(A);
    DevBuf<rocblas_int> info(2);
    info.zero(st);
    auto solver_guard = solver_lock();
    BlasHandle h(st);
    const bool ok = spd_inverse_device(h, d.p, n, info.p);
    DDPCA_HIP(hipStreamSynchronize(st));
    const auto inf = info.download();
    if (!ok) throw ApiError(DDPCA_EHIP, "rocsolver potrf/potri failed");
    if (inf[0] != 0 || inf[1] != 0) throw ApiError(DDPCA_ENUMERIC, "coarse operator is not positive definite");
    DDPCA_HIP(hipMemcpy(A.data(), d.p, A.size() * sizeof(double), hipMemcpyDeviceToHost));
}

bool inv_general_lu_device(std::vector<double>& A, int64_t n, hipStream_t st, double* resid) {
    DevBuf<double> d;
    d.upload(A);
    auto solver_guard = solver_lock();
    BlasHandle h(st);
    if (!inv_general_lu_device(h, d.p, n, resid)) return false;
    DDPCA_HIP(hipMemcpy(A.data(), d.p, A.size() * sizeof(double), hipMemcpyDeviceToHost));
    return true;
}

void pinv_general_device(std::vector<double>& A, int64_t n, hipStream_t st, int64_t* dropped) {
    DevBuf<double> d;
    d.upload(A);
    auto solver_guard = solver_lock();
    BlasHandle h(st);
    pinv_general_device(h, d.p, n, dropped);
    DDPCA_HIP(hipMemcpy(A.data(), d.p, A.size() * sizeof(double), hipMemcpyDeviceToHost));
}

}  // namespace ddpca
