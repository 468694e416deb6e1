// Thick-restart Lanczos on A^-1 for the eigenpairs of smallest magnitude of a symmetric positive
// definite A (MCONTACT::APPS, MCONTACT.h:2343-2403, runs Spectra's SymEigsSolver on globCoup_1 with
// SmallestMagn; here the inverse is on the device already, and the nev smallest eigenvalues of A
// are the reciprocals of the nev largest of A^-1).
//
// The basis V is column-major n x (ncv + 1) fp64 so the operator writes straight into the next
// column.  Every step orthogonalises the new column against all earlier ones by classical
// Gram-Schmidt, twice; the coefficients c = V^T w (summed over the two passes) are column j of the
// projected matrix T = V^T A^-1 V, kept on the device until a convergence check downloads them, so
// a step needs no host synchronisation.  T is diagonalised on the host (cyclic Jacobi, m <= 512);
// the Ritz vectors Y = V S of the nev largest Ritz values are tested on the TRUE residual of A,
// ||A y - theta y|| / theta with theta the Rayleigh quotient y.A y, every few steps.  At m = ncv
// the basis is compressed to nev + (ncv - nev) / 2 Ritz vectors and continued from the residual
// vector (thick restart, Wu & Simon 2000).
//
// Kernels (wave64): all reductions run in a fixed order with no atomics, so two calls give the
// same bits.  They are bandwidth-bound streams over V (n m 8 B per pass); DESIGN.md §3c has the
// byte model.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "../../include/ddpca_amd.h"
#include "device_eigs.hpp"

namespace ddpca {
namespace {

constexpr int kVtwTile = 256;   // rows of w one workgroup of k_eig_vtw stages in LDS
constexpr int kUpdTile = 64;    // rows per workgroup of k_eig_update (4 waves split the columns)
constexpr int kGemmCols = 8;    // output columns per workgroup of k_eig_gemm (S tile in LDS)

// fixed-order sum of one value per thread of a 256-thread workgroup (valid in thread 0)
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wsum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// start vector: a counter-based hash of the row index (splitmix64 finaliser), uniform in (-1, 1)
__global__ void k_eig_hash(double* v, int64_t n, uint64_t seed) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    v[i] = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// partial[j ntile + tile] = sum over the tile's rows of V[:, j] w, all m columns in one pass: the
// workgroup stages its row tile of w in LDS once and its waves sweep the columns (wave g of the
// 4 gridDim.y waves of a tile takes columns g, g + 4 gridDim.y, ...)
__global__ __launch_bounds__(256) void k_eig_vtw(const double* V, int64_t ld, int m, const double* w, int64_t n,
                                                 double* partial) {
    __shared__ double wl[kVtwTile];
    const int64_t row0 = (int64_t)blockIdx.x * kVtwTile;
    {
        const int64_t r = row0 + threadIdx.x;
        wl[threadIdx.x] = r < n ? w[r] : 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int stride = 4 * (int)gridDim.y;
    for (int j = (int)blockIdx.y * 4 + (threadIdx.x >> 6); j < m; j += stride) {
        const double* v = V + (int64_t)j * ld;
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < kVtwTile / 64; ++t) {
            const int64_t r = row0 + lane + 64 * t;
            if (r < n) s += v[r] * wl[lane + 64 * t];
        }
        s = wsum(s);
        if (lane == 0) partial[(int64_t)j * gridDim.x + blockIdx.x] = s;
    }
}

// c[j] = the tiles' partials of column j, one wavefront per column: lane l sums tiles l, l + 64,
// ... in order, then the fixed shuffle tree; tcol (column j of T) gets it, or adds it (second pass)
__global__ __launch_bounds__(256) void k_eig_vtw_fin(const double* partial, int ntile, int m, double* c, double* tcol,
                                                     int accumulate) {
    const int j = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= m) return;
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int t = lane; t < ntile; t += 64) s += partial[(int64_t)j * ntile + t];
    s = wsum(s);
    if (lane == 0) {
        c[j] = s;
        if (tcol) tcol[j] = accumulate ? tcol[j] + s : s;
    }
}

// w -= V c with c in LDS, fused with the partial sums of ||w||^2: 64 rows per workgroup, wave g
// takes columns g, g + 4, ...; the four shares are combined in a fixed order
__global__ __launch_bounds__(256) void k_eig_update(const double* V, int64_t ld, int m, const double* c, double* w, int64_t n,
                                                    double* npart) {
    __shared__ double cl[kEigsMaxNcv];
    __shared__ double sh[4][kUpdTile];
    for (int j = threadIdx.x; j < m; j += 256) cl[j] = c[j];
    __syncthreads();
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * kUpdTile + lane;
    double s = 0.0;
    if (r < n)
        for (int j = g; j < m; j += 4) s += V[(int64_t)j * ld + r] * cl[j];
    sh[g][lane] = s;
    __syncthreads();
    if (g == 0) {
        double a = 0.0;
        if (r < n) {
            a = w[r] - ((sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]));
            w[r] = a;
        }
        const double q = wsum(a * a);
        if (lane == 0) npart[blockIdx.x] = q;
    }
}

// beta[0] = sqrt of the partials' fixed-order sum (one workgroup)
__global__ __launch_bounds__(256) void k_eig_norm_fin(const double* npart, int nblk, double* beta) {
    __shared__ double red[4];
    double s = 0.0;
    for (int j = threadIdx.x; j < nblk; j += 256) s += npart[j];
    s = block_sum(s, red);
    if (threadIdx.x == 0) beta[0] = sqrt(s);
}

// w /= beta (the scalar stays on the device); a zero or non-finite norm leaves a zero column
__global__ void k_eig_scale(double* w, int64_t n, const double* beta) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double b = beta[0];
    w[i] = (b > 0.0 && b < 1.0e300) ? w[i] / b : 0.0;
}

// Y[:, c0 + cc] = V[:, :m] S[:, c0 + cc]: one row per thread, kGemmCols columns of S (m x k,
// column-major) in LDS
__global__ __launch_bounds__(256) void k_eig_gemm(const double* V, int64_t ld, int m, const double* S, int k, double* Y,
                                                  int64_t ldy, int64_t n) {
    __shared__ double sl[kEigsMaxNcv * kGemmCols];
    const int c0 = (int)blockIdx.y * kGemmCols;
    const int nc = min(kGemmCols, k - c0);
    for (int idx = threadIdx.x; idx < m * kGemmCols; idx += 256) {
        const int i = idx / kGemmCols, cc = idx % kGemmCols;
        sl[idx] = cc < nc ? S[(int64_t)(c0 + cc) * m + i] : 0.0;
    }
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    double acc[kGemmCols];
#pragma unroll
    for (int cc = 0; cc < kGemmCols; ++cc) acc[cc] = 0.0;
    for (int i = 0; i < m; ++i) {
        const double v = V[(int64_t)i * ld + r];
#pragma unroll
        for (int cc = 0; cc < kGemmCols; ++cc) acc[cc] += v * sl[i * kGemmCols + cc];
    }
#pragma unroll
    for (int cc = 0; cc < kGemmCols; ++cc)
        if (cc < nc) Y[(int64_t)(c0 + cc) * ldy + r] = acc[cc];
}

// AY[:, c] = A Y[:, c]: one wavefront per row, blockIdx.y the column
__global__ __launch_bounds__(256) void k_eig_csr(const int64_t* ptr, const int32_t* col, const double* val, int64_t n,
                                                 const double* Y, double* AY) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int lane = threadIdx.x & 63;
    const double* y = Y + (int64_t)blockIdx.y * n;
    double s = 0.0;
    for (int64_t q = ptr[r] + lane; q < ptr[r + 1]; q += 64) s += val[q] * y[col[q]];
    s = wsum(s);
    if (lane == 0) AY[(int64_t)blockIdx.y * n + r] = s;
}

// one workgroup per column: out[3c] = theta = y.Ay / y.y, out[3c + 1] = ||Ay - theta y|| / (|theta| ||y||),
// out[3c + 2] = ||y||
__global__ __launch_bounds__(256) void k_eig_resid(const double* Y, const double* AY, int64_t n, double* out) {
    __shared__ double red[4];
    __shared__ double bc[2];
    const double* y = Y + (int64_t)blockIdx.x * n;
    const double* ay = AY + (int64_t)blockIdx.x * n;
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        a += y[i] * ay[i];
        b += y[i] * y[i];
    }
    a = block_sum(a, red);
    b = block_sum(b, red);
    if (threadIdx.x == 0) {
        bc[0] = b > 0.0 ? a / b : 0.0;
        bc[1] = b;
    }
    __syncthreads();
    const double theta = bc[0];
    double q = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double d = ay[i] - theta * y[i];
        q += d * d;
    }
    q = block_sum(q, red);
    if (threadIdx.x == 0) {
        const double yn = sqrt(bc[1]);
        out[3 * blockIdx.x] = theta;
        out[3 * blockIdx.x + 1] = (theta != 0.0 && yn > 0.0) ? sqrt(q) / (fabs(theta) * yn) : 1.0e300;
        out[3 * blockIdx.x + 2] = yn;
    }
}

inline int nblk(int64_t n, int per) { return (int)std::max<int64_t>(1, (n + per - 1) / per); }

// HIP-event brackets summed per bucket after the stream synchronised
struct Stopwatch {
    bool on = false;
    hipStream_t st = nullptr;
    std::vector<hipEvent_t> pool;
    struct Span {
        size_t a, b;
        int bucket;
    };
    std::vector<Span> spans;
    size_t used = 0;
    size_t mark() {
        if (used == pool.size()) {
            hipEvent_t e = nullptr;
            DDPCA_HIP(hipEventCreate(&e));
            pool.push_back(e);
        }
        DDPCA_HIP(hipEventRecord(pool[used], st));
        return used++;
    }
    size_t open_ = 0;
    void begin() {
        if (on) open_ = mark();
    }
    void end(int bucket) {
        if (on) spans.push_back({open_, mark(), bucket});
    }
    void flush(double* ms) {  // after a stream synchronisation
        for (const Span& s : spans) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, pool[s.a], pool[s.b]) == hipSuccess) ms[s.bucket] += t;
        }
        spans.clear();
        used = 0;
    }
    ~Stopwatch() {
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    }
};

}  // namespace

void sym_eig_jacobi(int m, std::vector<double>& a, std::vector<double>& w, std::vector<double>& z) {
    z.assign((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) z[(size_t)i * m + i] = 1.0;
    auto A = [&](int i, int j) -> double& { return a[(size_t)i * m + j]; };
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int p = 0; p < m; ++p) {
            dia += A(p, p) * A(p, p);
            for (int q = p + 1; q < m; ++q) off += A(p, q) * A(p, q);
        }
        if (off == 0.0 || std::sqrt(2.0 * off) <= 1.0e-17 * std::sqrt(dia + 2.0 * off)) break;
        for (int p = 0; p < m - 1; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = A(p, q);
                if (apq == 0.0) continue;
                const double g = 100.0 * std::abs(apq);
                if (sweep > 3 && std::abs(A(p, p)) + g == std::abs(A(p, p)) && std::abs(A(q, q)) + g == std::abs(A(q, q))) {
                    A(p, q) = A(q, p) = 0.0;
                    continue;
                }
                const double th = (A(q, q) - A(p, p)) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::abs(th) + std::sqrt(th * th + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int r = 0; r < m; ++r) {  // columns p, q
                    const double rp = A(r, p), rq = A(r, q);
                    A(r, p) = c * rp - s * rq;
                    A(r, q) = s * rp + c * rq;
                }
                for (int r = 0; r < m; ++r) {  // rows p, q
                    const double pr = A(p, r), qr = A(q, r);
                    A(p, r) = c * pr - s * qr;
                    A(q, r) = s * pr + c * qr;
                }
                A(p, q) = A(q, p) = 0.0;
                for (int r = 0; r < m; ++r) {
                    const double zp = z[(size_t)r * m + p], zq = z[(size_t)r * m + q];
                    z[(size_t)r * m + p] = c * zp - s * zq;
                    z[(size_t)r * m + q] = s * zp + c * zq;
                }
            }
    }
    std::vector<int> ord(m);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return A(x, x) < A(y, y); });
    w.resize(m);
    std::vector<double> zs((size_t)m * m);
    for (int q = 0; q < m; ++q) {
        w[q] = A(ord[q], ord[q]);
        for (int r = 0; r < m; ++r) zs[(size_t)r * m + q] = z[(size_t)r * m + ord[q]];
    }
    z.swap(zs);
}

namespace {

// one Gram-Schmidt pass of column w against V[:, :m]: c = V^T w (into c, and into / onto tcol),
// w -= V c, npart = the partial sums of ||w||^2
void orth_pass(hipStream_t st, const double* V, int64_t n, int m, double* w, double* partial, double* c, double* tcol,
               bool accumulate, double* npart) {
    const int ntile = nblk(n, kVtwTile);
    const int ny = std::max(1, std::min(16, (m + 3) / 4));
    if (m > 0) {
        hipLaunchKernelGGL(k_eig_vtw, dim3(ntile, ny), dim3(256), 0, st, V, n, m, w, n, partial);
        hipLaunchKernelGGL(k_eig_vtw_fin, dim3(nblk(m, 4)), dim3(256), 0, st, partial, ntile, m, c, tcol, accumulate ? 1 : 0);
    }
    hipLaunchKernelGGL(k_eig_update, dim3(nblk(n, kUpdTile)), dim3(256), 0, st, V, n, m, c, w, n, npart);
}

}  // namespace

void eigs_smallest(hipStream_t st, int64_t n, const EigsApply& apply_inv, const EigsCsr& A, int nev, int ncv, double tol,
                   int64_t max_restarts, bool timed, double* Y, EigsResult& out) {
    if (nev < 1 || ncv <= nev || ncv > n || ncv > kEigsMaxNcv)
        throw ApiError(DDPCA_EINVAL, "eigs: need 1 <= nev < ncv <= min(n, " + std::to_string(kEigsMaxNcv) + ")");
    out = EigsResult();
    out.theta.assign(nev, 0.0);
    out.resid.assign(nev, 1.0e300);
    const int keep = nev + (ncv - nev) / 2;
    DevBuf<double> V((size_t)n * (ncv + 1)), tmp((size_t)n * std::max(keep, nev)), AY((size_t)n * nev);
    DevBuf<double> partial((size_t)nblk(n, kVtwTile) * (ncv + 1)), cdev(ncv + 1), tdev((size_t)ncv * ncv), beta(ncv + 1);
    DevBuf<double> npart(nblk(n, kUpdTile)), sdev((size_t)ncv * std::max(keep, nev)), rdev(3 * (size_t)nev);
    tdev.zero(st);
    beta.zero(st);
    Stopwatch sw;
    sw.on = timed;
    sw.st = st;
    auto col = [&](int j) { return V.p + (size_t)j * n; };
    auto normalise = [&](int j) {  // column j /= its norm (npart holds the partials), beta[j] = the norm
        hipLaunchKernelGGL(k_eig_norm_fin, dim3(1), dim3(256), 0, st, npart.p, nblk(n, kUpdTile), beta.p + j);
        hipLaunchKernelGGL(k_eig_scale, dim3(nblk(n, 256)), dim3(256), 0, st, col(j), n, beta.p + j);
    };
    // ---- start vector (never the load: whole families of modes can be orthogonal to it)
    sw.begin();
    hipLaunchKernelGGL(k_eig_hash, dim3(nblk(n, 256)), dim3(256), 0, st, col(0), n, (uint64_t)0x5DEECE66Dull);
    orth_pass(st, V.p, n, 0, col(0), partial.p, cdev.p, nullptr, false, npart.p);
    normalise(0);
    sw.end(1);

    std::vector<double> T((size_t)ncv * ncv, 0.0);  // host copy of the projected matrix, row-major
    int filled = 0;                                 // columns of T the host holds
    std::vector<double> mu, Z;                      // last host decomposition (of size mz)
    int mz = 0;
    int m = 0, last_check = 0;
    bool breakdown = false;

    // Ritz pairs of the current m columns; fills out.theta / out.resid / Y, returns max resid
    auto check = [&]() {
        DDPCA_HIP(hipStreamSynchronize(st));
        sw.flush(out.ms);
        if (m > filled) {
            std::vector<double> cols((size_t)(m - filled) * ncv), b(ncv + 1);
            {
                SyncCallGuard g;
                DDPCA_HIP(hipMemcpy(cols.data(), tdev.p + (size_t)filled * ncv, cols.size() * sizeof(double), hipMemcpyDeviceToHost));
                DDPCA_HIP(hipMemcpy(b.data(), beta.p, b.size() * sizeof(double), hipMemcpyDeviceToHost));
            }
            for (int j = filled; j < m; ++j)
                for (int i = 0; i <= j; ++i) T[(size_t)i * ncv + j] = T[(size_t)j * ncv + i] = cols[(size_t)(j - filled) * ncv + i];
            // an invariant subspace: the new column vanished, later columns carry nothing
            double scale = 0.0;
            for (int j = 0; j < m; ++j) scale = std::max(scale, std::abs(T[(size_t)j * ncv + j]));
            for (int j = filled; j < m; ++j)
                if (!(b[j + 1] > 1.0e-14 * scale)) {
                    m = j + 1;
                    breakdown = true;
                    break;
                }
            filled = m;
        }
        mz = m;
        std::vector<double> a((size_t)m * m);
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) a[(size_t)i * m + j] = T[(size_t)i * ncv + j];
        sym_eig_jacobi(m, a, mu, Z);
        const int k = std::min(nev, m);
        std::vector<double> S((size_t)m * k);  // column c: the Ritz vector of the c-th largest mu
        for (int c = 0; c < k; ++c)
            for (int i = 0; i < m; ++i) S[(size_t)c * m + i] = Z[(size_t)i * m + (m - 1 - c)];
        {
            SyncCallGuard g;
            DDPCA_HIP(hipMemcpy(sdev.p, S.data(), S.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        sw.begin();
        hipLaunchKernelGGL(k_eig_gemm, dim3(nblk(n, 256), nblk(k, kGemmCols)), dim3(256), 0, st, V.p, n, m, sdev.p, k, Y, n, n);
        hipLaunchKernelGGL(k_eig_csr, dim3(nblk(n, 4), k), dim3(256), 0, st, A.ptr, A.col, A.val, n, Y, AY.p);
        hipLaunchKernelGGL(k_eig_resid, dim3(k), dim3(256), 0, st, Y, AY.p, n, rdev.p);
        sw.end(2);
        DDPCA_HIP(hipStreamSynchronize(st));
        sw.flush(out.ms);
        std::vector<double> r(3 * (size_t)k);
        {
            SyncCallGuard g;
            DDPCA_HIP(hipMemcpy(r.data(), rdev.p, r.size() * sizeof(double), hipMemcpyDeviceToHost));
        }
        double worst = k < nev ? 1.0e300 : 0.0;
        for (int c = 0; c < k; ++c) {
            out.theta[c] = r[3 * c];
            out.resid[c] = r[3 * c + 1];
            if (!std::isfinite(out.resid[c])) out.resid[c] = 1.0e300;  // not converged
            worst = std::max(worst, out.resid[c]);
        }
        last_check = m;
        return worst;
    };

    for (;;) {
        while (m < ncv && !breakdown) {
            const int j = m;
            sw.begin();
            apply_inv(col(j), col(j + 1));
            sw.end(0);
            ++out.applies;
            sw.begin();
            double* tcol = tdev.p + (size_t)j * ncv;
            orth_pass(st, V.p, n, j + 1, col(j + 1), partial.p, cdev.p, tcol, false, npart.p);
            orth_pass(st, V.p, n, j + 1, col(j + 1), partial.p, cdev.p, tcol, true, npart.p);
            normalise(j + 1);
            sw.end(1);
            ++m;
            ++out.steps;
            if (m >= nev && (m == ncv || m - last_check >= std::max(5, m / 4))) {
                const double worst = check();
                if (worst <= tol) {
                    out.converged = true;
                    break;
                }
            }
        }
        if (out.converged) break;
        if (breakdown) {  // the Krylov space is exhausted: what it holds is all there is
            if (last_check != m) out.converged = check() <= tol;
            break;
        }
        if (out.restarts >= max_restarts) break;
        // ---- thick restart: V[:, :keep] = V[:, :ncv] S_keep, then the residual vector
        std::vector<double> S((size_t)ncv * keep);
        for (int c = 0; c < keep; ++c)
            for (int i = 0; i < ncv; ++i) S[(size_t)c * ncv + i] = Z[(size_t)i * mz + (ncv - 1 - c)];
        {
            SyncCallGuard g;
            DDPCA_HIP(hipMemcpy(sdev.p, S.data(), S.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        sw.begin();
        hipLaunchKernelGGL(k_eig_gemm, dim3(nblk(n, 256), nblk(keep, kGemmCols)), dim3(256), 0, st, V.p, n, ncv, sdev.p, keep,
                           tmp.p, n, n);
        DDPCA_HIP(hipMemcpyAsync(V.p, tmp.p, (size_t)n * keep * sizeof(double), hipMemcpyDeviceToDevice, st));
        DDPCA_HIP(hipMemcpyAsync(col(keep), col(ncv), (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
        sw.end(2);
        std::fill(T.begin(), T.end(), 0.0);
        for (int c = 0; c < keep; ++c) T[(size_t)c * ncv + c] = mu[ncv - 1 - c];
        filled = keep;
        m = keep;
        last_check = m;
        ++out.restarts;
    }
    DDPCA_HIP(hipStreamSynchronize(st));
    sw.flush(out.ms);
    // ascending theta (descending mu already, but the Rayleigh quotients decide)
    std::vector<int> ord(nev);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return out.theta[a] < out.theta[b]; });
    bool sorted = true;
    for (int c = 0; c < nev; ++c) sorted = sorted && ord[c] == c;
    if (!sorted) {
        DDPCA_HIP(hipMemcpyAsync(tmp.p, Y, (size_t)n * nev * sizeof(double), hipMemcpyDeviceToDevice, st));
        std::vector<double> th(nev), rs(nev);
        for (int c = 0; c < nev; ++c) {
            DDPCA_HIP(hipMemcpyAsync(Y + (size_t)c * n, tmp.p + (size_t)ord[c] * n, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
            th[c] = out.theta[ord[c]];
            rs[c] = out.resid[ord[c]];
        }
        out.theta = th;
        out.resid = rs;
        DDPCA_HIP(hipStreamSynchronize(st));
    }
}

void eigs_orth_bench(int device, int64_t n, int m, int reps, double out[4]) {
    if (n < 1 || m < 1 || m > kEigsMaxNcv || reps < 1) throw ApiError(DDPCA_EINVAL, "eigs_orth_bench: arguments");
    select_device(device);
    hipStream_t st = nullptr;
    DDPCA_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipEvent_t e[2] = {nullptr, nullptr};
    try {
        DevBuf<double> V((size_t)n * (m + 1)), partial(std::max<size_t>((size_t)nblk(n, kVtwTile) * m, 12 * 1024)), cdev(m),
            npart(nblk(n, kUpdTile));
        std::vector<double> chost(m);
        for (int j = 0; j <= m; ++j)
            hipLaunchKernelGGL(k_eig_hash, dim3(nblk(n, 256)), dim3(256), 0, st, V.p + (size_t)j * n, n, (uint64_t)(j + 1));
        for (auto& x : e) DDPCA_HIP(hipEventCreate(&x));
        double* w = V.p + (size_t)m * n;
        for (int variant = 0; variant < 2; ++variant) {
            auto pass = [&] {
                if (variant == 0) orth_pass(st, V.p, n, m, w, partial.p, cdev.p, nullptr, false, npart.p);
                else krylov_cgs_pass(st, n, V.p, n, m, w, partial.p, cdev.p, chost.data());
            };
            pass();  // warm-up
            DDPCA_HIP(hipStreamSynchronize(st));
            DDPCA_HIP(hipEventRecord(e[0], st));
            for (int r = 0; r < reps; ++r) pass();
            DDPCA_HIP(hipEventRecord(e[1], st));
            DDPCA_HIP(hipStreamSynchronize(st));
            float ms = 0.f;
            DDPCA_HIP(hipEventElapsedTime(&ms, e[0], e[1]));
            out[variant] = (double)ms / reps;
        }
        // algorithmic bytes of one pass: V twice (the dots, the update), w read by the dots, read
        // and written by the update, the coefficients
        out[2] = 2.0 * 8.0 * (double)n * m + 24.0 * (double)n + 16.0 * m;
        out[3] = 0.0;
    } catch (...) {
        for (auto& x : e)
            if (x) (void)hipEventDestroy(x);
        (void)hipStreamDestroy(st);
        throw;
    }
    for (auto& x : e) (void)hipEventDestroy(x);
    (void)hipStreamDestroy(st);
}

}  // namespace ddpca
