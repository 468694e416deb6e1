// Stress recovery on the device (gfx950, fp64 throughout): MULTIGRID::STRESS_RECOVERY,
// MULTIGRID.h:1316-1433, from the plan of MULTIGRID::STRESS_PLAN (stress.cpp restates the same
// arithmetic on the host; both share stress_elem.hpp).
//
//   k_stress_elem  8 lanes per leaf element, a wavefront 8 elements.  Lane j gathers corner j
//                  (coordinates, displacement, rotated for a nodeRota node), the group exchanges
//                  the corners with shuffles of width 8 and every lane keeps the modal
//                  coefficients of the geometry and the displacement (2 x 24 doubles).  The 27
//                  Gauss points are evaluated by all 8 lanes alike; lane j accumulates row j of
//                  M = sum w |J| N^T N (8) and of F = sum w |J| N^T sigma^T (6).  M^-1 F is a
//                  Gauss-Jordan elimination without pivoting (M is symmetric positive definite)
//                  over the 8 lanes: step k broadcasts lane k's row, every lane eliminates its
//                  own.  Row j of the element's nodal stresses leaves from lane j: 48 doubles per
//                  element, contiguous per group.  No LDS, no scratch.
//   k_stress_node  one thread per node: its contributions (leaf, corner mask) in the plan's fixed
//                  order, each the mean of the masked rows, summed from zero, divided by the
//                  count (0 / 0 = NaN for a node without contribution, as in the reference), then
//                  the von Mises stress: 7 doubles.  A gather, no atomics: bit-identical run to
//                  run.
// Byte model and resource usage: DESIGN.md "Stress recovery".
#include "device_stress.hpp"

#include <mutex>

#include "device_common.hpp"
#include "stress_elem.hpp"

namespace ddpca {

namespace {

constexpr int kGroup = 8;  // lanes per element

__global__ __launch_bounds__(kBlock) void k_stress_elem(int64_t nleaf, const int32_t* __restrict__ corner,
                                                        const double* __restrict__ coords,
                                                        const double* __restrict__ u_main,
                                                        const double* __restrict__ u_hang, int64_t nsplit,
                                                        const int32_t* __restrict__ rotIndex,
                                                        const double* __restrict__ rot, double lam, double mu,
                                                        double* __restrict__ se) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int j = threadIdx.x & (kGroup - 1);
    int64_t l = t / kGroup;
    // a group past the end repeats the last element (every lane stays in the shuffles) and stores nothing
    const bool live = l < nleaf;
    if (!live) l = nleaf - 1;
    const int64_t n = corner[kGroup * l + j];
    double xo[3], uo[3];
    {
        const double* up = n < nsplit ? u_main + 3 * n : u_hang + 3 * (n - nsplit);
        const double a = up[0], b = up[1], c = up[2];
        const int32_t r = rotIndex[n];
        uo[0] = a, uo[1] = b, uo[2] = c;
        if (r >= 0) {
            const double* R = rot + 9 * (int64_t)r;
            for (int i = 0; i < 3; ++i) uo[i] = R[3 * i] * a + R[3 * i + 1] * b + R[3 * i + 2] * c;
        }
        for (int i = 0; i < 3; ++i) xo[i] = coords[3 * n + i];
    }
    double C[8][3], U[8][3];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[i][c] = U[i][c] = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        double xk[3], uk[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xk[c] = __shfl(xo[c], k, kGroup);
            uk[c] = __shfl(uo[c], k, kGroup);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                C[i][c] += stress::mode_sign(i, k) * xk[c];
                U[i][c] += stress::mode_sign(i, k) * uk[c];
            }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[i][c] *= 0.125, U[i][c] *= 0.125;

    const double sx = stress::sgn_xi(j), sy = stress::sgn_eta(j), sz = stress::sgn_zeta(j);
    double M[8], F[6];
#pragma unroll
    for (int k = 0; k < 8; ++k) M[k] = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) F[c] = 0.0;
#pragma unroll 1
    for (int gi = 0; gi < 3; ++gi)
#pragma unroll 1
        for (int gj = 0; gj < 3; ++gj)
#pragma unroll 1
            for (int gk = 0; gk < 3; ++gk) {
                const double x = stress::gauss_pt(gi), y = stress::gauss_pt(gj), z = stress::gauss_pt(gk);
                double sig[6];
                const double det = stress::gauss_stress(C, U, x, y, z, lam, mu, sig);
                const double w = stress::gauss_wt(gi) * stress::gauss_wt(gj) * stress::gauss_wt(gk) * det;
                const double wn = w * stress::shape(sx, sy, sz, x, y, z);
#pragma unroll
                for (int c = 0; c < 6; ++c) F[c] += wn * sig[c];
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    M[k] += wn * stress::shape(stress::sgn_xi(k), stress::sgn_eta(k), stress::sgn_zeta(k), x, y, z);
            }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double rinv = 1.0 / __shfl(M[k], k, kGroup);
        const double f = M[k];
        const bool piv = j == k;
#pragma unroll
        for (int c = k + 1; c < 8; ++c) {
            const double p = __shfl(M[c], k, kGroup) * rinv;
            M[c] = piv ? p : M[c] - f * p;
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double p = __shfl(F[c], k, kGroup) * rinv;
            F[c] = piv ? p : F[c] - f * p;
        }
    }
    if (live) {
        double* o = se + 48 * l + 6 * j;
#pragma unroll
        for (int c = 0; c < 6; ++c) o[c] = F[c];
    }
}

__global__ __launch_bounds__(kBlock) void k_stress_node(int64_t nnode, const int64_t* __restrict__ ptr,
                                                        const int32_t* __restrict__ leaf,
                                                        const uint8_t* __restrict__ mask,
                                                        const double* __restrict__ se, double* __restrict__ stre) {
    const int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (n >= nnode) return;
    const int64_t q0 = ptr[n], q1 = ptr[n + 1];
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t q = q0; q < q1; ++q) {
        double m[6];
        stress::masked_mean(se + 48 * (int64_t)leaf[q], mask[q], m);
#pragma unroll
        for (int c = 0; c < 6; ++c) s[c] += m[c];
    }
    const double cnt = (double)(q1 - q0);
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c] = s[c] / cnt;
    double* o = stre + 7 * n;
#pragma unroll
    for (int c = 0; c < 6; ++c) o[c] = s[c];
    o[6] = sqrt(stress::von_mises_sq(s));
}

// the plan on one device (StressPlan::device)
struct StressDev {
    int device = -1;
    DevBuf<int32_t> corner, leaf, rotIndex;
    DevBuf<uint8_t> mask;
    DevBuf<int64_t> ptr;
    DevBuf<double> coords, rot, se, stre;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // around k_stress_elem and k_stress_node of the last call
    ~StressDev() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

std::mutex& upload_mutex() {
    static std::mutex m;
    return m;
}

}  // namespace

const double* stress_device(MULTIGRID& g, int device, const double* u_main, const double* u_hang, int64_t nsplit,
                            hipStream_t stream) {
    const StressPlan& P = g.STRESS_PLAN();
    std::lock_guard<std::mutex> lock(upload_mutex());
    auto D = std::static_pointer_cast<StressDev>(g.strePlan->device);
    if (!D || D->device != device) {
        D = std::make_shared<StressDev>();
        D->device = device;
        D->corner.upload(P.corner);
        D->leaf.upload(P.leaf);
        D->mask.upload(P.mask);
        D->ptr.upload(P.ptr);
        D->rotIndex.upload(P.rotIndex);
        // never a null pointer in the kernel's arguments: one unused block without rotations
        D->rot.upload(P.rot.empty() ? std::vector<double>(9, 0.0) : P.rot);
        std::vector<double> xyz((size_t)3 * P.nnode);
        for (int64_t i = 0; i < P.nnode; ++i)
            for (int a = 0; a < 3; ++a) xyz[3 * i + a] = g.nodeCoor[i][a];
        D->coords.upload(xyz);
        D->se.alloc((size_t)48 * P.nleaf);
        D->stre.alloc((size_t)7 * P.nnode);
        for (hipEvent_t& e : D->ev) DDPCA_HIP(hipEventCreate(&e));
        g.strePlan->device = D;
    }
    if (nsplit < 0 || nsplit > P.nnode) throw ApiError(DDPCA_EINVAL, "stress: displacement ranges outside the nodes");
    const double lam = g.mateElas * g.matePois / (1.0 + g.matePois) / (1.0 - 2.0 * g.matePois);
    const double mu = g.mateElas / 2.0 / (1.0 + g.matePois);
    DDPCA_HIP(hipEventRecord(D->ev[0], stream));
    if (P.nleaf > 0)
        hipLaunchKernelGGL(k_stress_elem, dim3(ceil_div(P.nleaf * kGroup, kBlock)), dim3(kBlock), 0, stream, P.nleaf,
                           D->corner.p, D->coords.p, u_main, u_hang, nsplit, D->rotIndex.p, D->rot.p, lam, mu, D->se.p);
    DDPCA_HIP(hipEventRecord(D->ev[1], stream));
    hipLaunchKernelGGL(k_stress_node, dim3(ceil_div(P.nnode, kBlock)), dim3(kBlock), 0, stream, P.nnode, D->ptr.p,
                       D->leaf.p, D->mask.p, D->se.p, D->stre.p);
    DDPCA_HIP(hipGetLastError());
    DDPCA_HIP(hipEventRecord(D->ev[2], stream));
    return D->stre.p;
}

void stress_kernel_ms(MULTIGRID& g, double out[2]) {
    out[0] = out[1] = 0.0;
    std::lock_guard<std::mutex> lock(upload_mutex());
    if (!g.strePlan || !g.strePlan->device) return;
    auto D = std::static_pointer_cast<StressDev>(g.strePlan->device);
    for (int k = 0; k < 2; ++k) {
        float ms = 0.0f;
        DDPCA_HIP(hipEventElapsedTime(&ms, D->ev[k], D->ev[k + 1]));
        out[k] = ms;
    }
}

}  // namespace ddpca
