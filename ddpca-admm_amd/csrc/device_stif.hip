// Stiffness assembly on the device (gfx950, fp64 throughout): the element loop of
// MULTIGRID::STIF_MATR, MULTIGRID.h:950-1039, and MULTIGRID::GET_VOLUME, MULTIGRID.h:1041-1082,
// from the plan of MULTIGRID::STIF_PLAN (multigrid.cpp; the pattern is the host's own).
//
//   k_stif_elem    8 lanes per leaf element, a wavefront 8 elements.  Lane a gathers corner a's
//                  coordinates, the group exchanges them with shuffles of width 8 and every lane
//                  keeps the modal coefficients of the trilinear geometry (modes 1-7, 21 doubles).
//                  All 8 lanes evaluate J, det J and J^-1 at the 27 Gauss points alike; with
//                  d_n = J^-1 grad N_n and f = w_g det J lane a accumulates S_ab = sum_g f d_a d_b^T
//                  for b = 0..7 (72 accumulators, every index a compile-time constant) and forms
//                  K_ab = lam S_ab + mu S_ab^T + mu tr(S_ab) I at the end: block row a of the
//                  element matrix, 72 contiguous doubles.  Every block is stored (576 doubles per
//                  element); lane 0 stores the element's volume sum_g f.  No LDS, no scratch.
//   k_stif_gather  one thread per stored block (row node r, column node c): r's incident leaves in
//                  ascending order (the order the host's general path adds them in), the local
//                  corner b with corner[b] == c by 8 compares, 9 accumulators summed from zero,
//                  stored row-major in Bsr3::val's layout.  A gather, no atomics: bit-identical
//                  run to run.
//   k_stif_vol_part / k_stif_vol_fin   the volume: one wavefront per chunk of 4096 elements (lane i
//                  sums elements i, i + 64, ... of its chunk in index order, then a fixed shuffle
//                  tree), then one wavefront over the chunk partials the same way.
// Byte model and resource usage: DESIGN.md "Stiffness assembly".
#include "device_stif.hpp"

#include <chrono>
#include <mutex>

#include "device_common.hpp"
#include "stress_elem.hpp"

namespace ddpca {

namespace {

constexpr int kGroup = 8;         // lanes per element
constexpr int kVolChunk = 4096;   // elements per volume partial

// kStif = false: the volume alone (GET_VOLUME), no stiffness accumulators.  Two waves per SIMD is
// asked for: left alone the register allocator takes 256 VGPRs + 24 AGPRs and one wave.
template <bool kStif>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2))) void k_stif_elem(
    int64_t nleaf, const int32_t* __restrict__ corner, const double* __restrict__ coords, double lam, double mu,
    double* __restrict__ ke, double* __restrict__ vol) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int a = threadIdx.x & (kGroup - 1);
    int64_t l = t / kGroup;
    // a group past the end repeats the last element (every lane stays in the shuffles) and stores nothing
    const bool live = l < nleaf;
    if (!live) l = nleaf - 1;
    const int64_t n = corner[kGroup * l + a];
    double xo[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) xo[c] = coords[3 * n + c];
    // modal coefficients 1..7 of the geometry (stress_elem.hpp): C[m - 1] = 1/8 sum_k s_m(k) X_k
    double C[7][3];
#pragma unroll
    for (int m = 0; m < 7; ++m)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[m][c] = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        double xk[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) xk[c] = __shfl(xo[c], k, kGroup);
#pragma unroll
        for (int m = 0; m < 7; ++m)
#pragma unroll
            for (int c = 0; c < 3; ++c) C[m][c] += stress::mode_sign(m + 1, k) * xk[c];
    }
#pragma unroll
    for (int m = 0; m < 7; ++m)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[m][c] *= 0.125;
    if (!live) return;  // past the shuffles: nothing below crosses lanes

    const double sx = stress::sgn_xi(a), sy = stress::sgn_eta(a), sz = stress::sgn_zeta(a);
    double S[8][3][3];
    if (kStif) {
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) S[b][i][j] = 0.0;
    }
    double v = 0.0;
    // one rolled loop over the 27 points: nested loops let the compiler keep partial sums of J
    // across the inner ones, which costs the registers that hold the kernel at 2 waves per SIMD
#pragma unroll 1
    for (int g = 0; g < 27; ++g) {
        const int gi = g / 9, gj = g / 3 % 3, gk = g % 3;
        const double x = stress::gauss_pt(gi), y = stress::gauss_pt(gj), z = stress::gauss_pt(gk);
        const double yz = y * z, xz = x * z, xy = x * y;
        double J[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            J[0][c] = fma(C[6][c], yz, fma(C[5][c], z, fma(C[3][c], y, C[0][c])));
            J[1][c] = fma(C[6][c], xz, fma(C[4][c], z, fma(C[3][c], x, C[1][c])));
            J[2][c] = fma(C[6][c], xy, fma(C[5][c], x, fma(C[4][c], y, C[2][c])));
        }
        double A[3][3];  // adj(J), A[c][r] = cofactor of J[r][c]
        A[0][0] = fma(J[1][1], J[2][2], -(J[1][2] * J[2][1]));
        A[0][1] = fma(J[0][2], J[2][1], -(J[0][1] * J[2][2]));
        A[0][2] = fma(J[0][1], J[1][2], -(J[0][2] * J[1][1]));
        A[1][0] = fma(J[1][2], J[2][0], -(J[1][0] * J[2][2]));
        A[1][1] = fma(J[0][0], J[2][2], -(J[0][2] * J[2][0]));
        A[1][2] = fma(J[0][2], J[1][0], -(J[0][0] * J[1][2]));
        A[2][0] = fma(J[1][0], J[2][1], -(J[1][1] * J[2][0]));
        A[2][1] = fma(J[0][1], J[2][0], -(J[0][0] * J[2][1]));
        A[2][2] = fma(J[0][0], J[1][1], -(J[0][1] * J[1][0]));
        const double det = fma(J[0][2], A[2][0], fma(J[0][1], A[1][0], J[0][0] * A[0][0]));
        const double f = stress::gauss_wt(gi) * stress::gauss_wt(gj) * stress::gauss_wt(gk) * det;
        v += f;
        if (kStif) {
            const double r = 1.0 / det;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int q = 0; q < 3; ++q) A[c][q] *= r;  // J^-1
            // (1 -+ x) / 2 and so on: grad N_n = (sx ay az, ax sy az, ax ay sz) / 2 with the
            // factors of corner n's signs
            const double ax[2] = {0.5 * (1.0 - x), 0.5 * (1.0 + x)};
            const double ay[2] = {0.5 * (1.0 - y), 0.5 * (1.0 + y)};
            const double az[2] = {0.5 * (1.0 - z), 0.5 * (1.0 + z)};
            double fa[3];
            {
                const double px = sx > 0.0 ? ax[1] : ax[0], py = sy > 0.0 ? ay[1] : ay[0], pz = sz > 0.0 ? az[1] : az[0];
                const double g0 = 0.5 * sx * (py * pz), g1 = 0.5 * sy * (px * pz), g2 = 0.5 * sz * (px * py);
#pragma unroll
                for (int c = 0; c < 3; ++c) fa[c] = f * fma(A[c][2], g2, fma(A[c][1], g1, A[c][0] * g0));
            }
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int ix = stress::sgn_xi(b) > 0.0, iy = stress::sgn_eta(b) > 0.0, iz = stress::sgn_zeta(b) > 0.0;
                const double g0 = (ix ? 0.5 : -0.5) * (ay[iy] * az[iz]);
                const double g1 = (iy ? 0.5 : -0.5) * (ax[ix] * az[iz]);
                const double g2 = (iz ? 0.5 : -0.5) * (ax[ix] * ay[iy]);
                double db[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) db[c] = fma(A[c][2], g2, fma(A[c][1], g1, A[c][0] * g0));
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) S[b][i][j] = fma(fa[i], db[j], S[b][i][j]);
            }
        }
    }
    if (a == 0) vol[l] = v;
    if (kStif) {
        double* o = ke + (int64_t)kStifElemDoubles * l + 72 * a;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const double tr = mu * ((S[b][0][0] + S[b][1][1]) + S[b][2][2]);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double k = fma(lam, S[b][i][j], mu * S[b][j][i]);
                    o[9 * b + 3 * i + j] = i == j ? k + tr : k;
                }
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_stif_gather(int64_t nnzb, const int32_t* __restrict__ brow,
                                                        const int32_t* __restrict__ col,
                                                        const int64_t* __restrict__ n2e_ptr,
                                                        const int32_t* __restrict__ n2e_inc,
                                                        const int32_t* __restrict__ corner,
                                                        const double* __restrict__ ke, double* __restrict__ val) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= nnzb) return;
    const int32_t r = brow[p], c = col[p];
    double acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.0;
    const int64_t q1 = n2e_ptr[r + 1];
    for (int64_t q = n2e_ptr[r]; q < q1; ++q) {
        const int32_t inc = n2e_inc[q];
        const int64_t l = inc >> 3;
        const int a = inc & 7;
        const int4* cp = reinterpret_cast<const int4*>(corner + 8 * l);
        const int4 c0 = cp[0], c1 = cp[1];
        const int32_t cn[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        const double* e = ke + (int64_t)kStifElemDoubles * l + 72 * a;
#pragma unroll
        for (int b = 0; b < 8; ++b)
            if (cn[b] == c) {
#pragma unroll
                for (int i = 0; i < 9; ++i) acc[i] += e[9 * b + i];
            }
    }
    double* o = val + 9 * p;
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = acc[i];
}

__device__ __forceinline__ double wave_tree(double s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
    return s;
}

// part[chunk] = the volumes of elements [chunk * kVolChunk, ...), one wavefront per chunk
__global__ __launch_bounds__(kWave) void k_stif_vol_part(int64_t nleaf, const double* __restrict__ vol,
                                                         double* __restrict__ part) {
    const int64_t base = (int64_t)blockIdx.x * kVolChunk;
    double s = 0.0;
    for (int k = 0; k < kVolChunk / kWave; ++k) {
        const int64_t i = base + (int64_t)k * kWave + threadIdx.x;
        if (i < nleaf) s += vol[i];
    }
    s = wave_tree(s);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kWave) void k_stif_vol_fin(int64_t npart, const double* __restrict__ part,
                                                        double* __restrict__ out) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < npart; i += kWave) s += part[i];
    s = wave_tree(s);
    if (threadIdx.x == 0) out[0] = s;
}

// the plan on one device (StifPlan::device)
struct StifDev {
    int device = -1;
    DevBuf<int32_t> corner, brow, col, n2e_inc;
    DevBuf<int64_t> n2e_ptr;
    DevBuf<double> coords;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // around k_stif_elem and k_stif_gather of the last call
    ~StifDev() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

std::mutex& upload_mutex() {
    static std::mutex m;
    return m;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the cached device copy of g's plan (made on first use; *upload_ms = the host clock of making it)
std::shared_ptr<StifDev> plan_on_device(MULTIGRID& g, const StifPlan& P, int device, double* upload_ms) {
    auto D = std::static_pointer_cast<StifDev>(g.stifPlan->device);
    *upload_ms = 0.0;
    if (D && D->device == device) return D;
    const auto t0 = std::chrono::steady_clock::now();
    D = std::make_shared<StifDev>();
    D->device = device;
    D->corner.upload(P.corner);
    D->brow.upload(P.brow);
    D->col.upload(P.K.col);
    D->n2e_ptr.upload(P.n2ePtr);
    D->n2e_inc.upload(P.n2eInc);
    std::vector<double> xyz((size_t)3 * P.nnode);
    for (int64_t i = 0; i < P.nnode; ++i)
        for (int a = 0; a < 3; ++a) xyz[3 * i + a] = g.nodeCoor[i][a];
    D->coords.upload(xyz);
    for (hipEvent_t& e : D->ev) DDPCA_HIP(hipEventCreate(&e));
    g.stifPlan->device = D;
    *upload_ms = ms_since(t0);
    return D;
}

// a device allocation that names its size when it fails (no host fallback)
template <typename T>
void alloc_or_explain(DevBuf<T>& b, size_t count, const char* what) {
    try {
        b.alloc(count);
    } catch (const ApiError& e) {
        (void)hipGetLastError();
        throw ApiError(e.code, std::string("stiffness assembly: ") + what + " needs " + std::to_string(count * sizeof(T)) +
                                   " bytes of device memory (" + e.what() + ")");
    }
}

double reduce_volume(int64_t nleaf, const double* vol) {
    const int64_t npart = (nleaf + kVolChunk - 1) / kVolChunk;
    DevBuf<double> part((size_t)npart + 1);
    hipLaunchKernelGGL(k_stif_vol_part, dim3((unsigned)npart), dim3(kWave), 0, nullptr, nleaf, vol, part.p);
    hipLaunchKernelGGL(k_stif_vol_fin, dim3(1), dim3(kWave), 0, nullptr, npart, part.p, part.p + npart);
    DDPCA_HIP(hipGetLastError());
    DDPCA_HIP(hipStreamSynchronize(nullptr));
    double v = 0.0;
    SyncCallGuard guard;
    DDPCA_HIP(hipMemcpy(&v, part.p + npart, sizeof(double), hipMemcpyDeviceToHost));
    return v;
}

}  // namespace

void stif_device(MULTIGRID& g, int device, double* val, double* volume, double ms[4]) {
    const StifPlan& P = g.STIF_PLAN();
    std::lock_guard<std::mutex> lock(upload_mutex());
    double upload_ms = 0.0;
    auto D = plan_on_device(g, P, device, &upload_ms);
    const double lam = g.mateElas * g.matePois / (1.0 + g.matePois) / (1.0 - 2.0 * g.matePois);
    const double mu = g.mateElas / 2.0 / (1.0 + g.matePois);
    const int64_t nnzb = P.K.nnzb();
    DevBuf<double> ke, vol, dval;
    alloc_or_explain(ke, (size_t)kStifElemDoubles * P.nleaf, "the element matrices");
    alloc_or_explain(vol, (size_t)P.nleaf, "the element volumes");
    alloc_or_explain(dval, (size_t)9 * nnzb, "the assembled blocks");
    DDPCA_HIP(hipEventRecord(D->ev[0], nullptr));
    hipLaunchKernelGGL(k_stif_elem<true>, dim3(ceil_div(P.nleaf * kGroup, kBlock)), dim3(kBlock), 0, nullptr, P.nleaf,
                       D->corner.p, D->coords.p, lam, mu, ke.p, vol.p);
    DDPCA_HIP(hipEventRecord(D->ev[1], nullptr));
    hipLaunchKernelGGL(k_stif_gather, dim3(ceil_div(nnzb, kBlock)), dim3(kBlock), 0, nullptr, nnzb, D->brow.p, D->col.p,
                       D->n2e_ptr.p, D->n2e_inc.p, D->corner.p, ke.p, dval.p);
    DDPCA_HIP(hipGetLastError());
    DDPCA_HIP(hipEventRecord(D->ev[2], nullptr));
    const double v = reduce_volume(P.nleaf, vol.p);  // synchronises the stream
    if (volume) *volume = v;
    const auto t0 = std::chrono::steady_clock::now();
    {
        SyncCallGuard guard;
        DDPCA_HIP(hipMemcpy(val, dval.p, (size_t)9 * nnzb * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (ms) {
        for (int k = 0; k < 2; ++k) {
            float e = 0.0f;
            DDPCA_HIP(hipEventElapsedTime(&e, D->ev[k], D->ev[k + 1]));
            ms[k] = e;
        }
        ms[2] = upload_ms;
        ms[3] = ms_since(t0);
    }
}

double volume_device(MULTIGRID& g, int device) {
    const StifPlan& P = g.STIF_PLAN();
    std::lock_guard<std::mutex> lock(upload_mutex());
    double upload_ms = 0.0;
    auto D = plan_on_device(g, P, device, &upload_ms);
    DevBuf<double> vol;
    alloc_or_explain(vol, (size_t)P.nleaf, "the element volumes");
    hipLaunchKernelGGL(k_stif_elem<false>, dim3(ceil_div(P.nleaf * kGroup, kBlock)), dim3(kBlock), 0, nullptr, P.nleaf,
                       D->corner.p, D->coords.p, 0.0, 0.0, nullptr, vol.p);
    DDPCA_HIP(hipGetLastError());
    return reduce_volume(P.nleaf, vol.p);
}

}  // namespace ddpca
