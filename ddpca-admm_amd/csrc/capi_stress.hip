// C ABI of the stress recovery (MULTIGRID::STRESS_RECOVERY, MULTIGRID.h:1316-1433):
// ddpca_multigrid_stress on a built element tree (device kernels, or the host restatement for
// device < 0) and mcontact_gpu_stress from an MCONTACT handle's device-resident resuDisp.
#include <algorithm>

#include "../../include/ddpca_amd.h"
#include "device_common.hpp"
#include "device_stress.hpp"
#include "problem.hpp"

using namespace ddpca;

namespace {
thread_local double last_kernel_ms[2] = {0.0, 0.0};
}

extern "C" {

int ddpca_stress_last_kernel_ms(double* out2) {
    return guarded([&] {
        if (!out2) throw ApiError(DDPCA_EINVAL, "ddpca_stress_last_kernel_ms: null argument");
        out2[0] = last_kernel_ms[0];
        out2[1] = last_kernel_ms[1];
    });
}

// MULTIGRID.h:1316-1433
int ddpca_multigrid_stress(ddpca_multigrid_t h, int device, const double* disp, double* stre) {
    return guarded([&] {
        bool built = false;
        MULTIGRID* g = multigrid_of(h, &built);
        if (!g || !disp || !stre) throw ApiError(DDPCA_EINVAL, "ddpca_multigrid_stress: null argument");
        if (!built) throw ApiError(DDPCA_EINVAL, "ddpca_multigrid_stress: ddpca_multigrid_build has not run");
        try {
            if (device < 0) {
                g->STRESS_RECOVERY(disp, stre);
                return;
            }
            select_device(device);
            const int64_t N = g->STRESS_PLAN().nnode;
            DevBuf<double> u;
            u.upload(disp, (size_t)3 * N);
            const double* out = stress_device(*g, device, u.p, u.p + 3 * N, N, nullptr);
            DDPCA_HIP(hipStreamSynchronize(nullptr));
            stress_kernel_ms(*g, last_kernel_ms);
            SyncCallGuard guard;
            DDPCA_HIP(hipMemcpy(stre, out, (size_t)7 * N * sizeof(double), hipMemcpyDeviceToHost));
        } catch (const std::invalid_argument& e) {
            throw ApiError(DDPCA_EINVAL, e.what());
        }
    });
}

// MULTIGRID.h:1316-1433
int64_t mcontact_gpu_stress(mcontact_t h, ddpca_problem_t p, int64_t tv, double* out, int64_t cap) {
    int64_t n = 0;
    const int rc = guarded([&] {
        if (!h || !p) throw ApiError(DDPCA_EINVAL, "mcontact_gpu_stress: handle / problem");
        Problem& P = *reinterpret_cast<Problem*>(p);
        SubDisp S;
        if (tv < 0 || tv >= (int64_t)P.mc.multGrid.size() || !mcontact_sub_disp(h, tv, &S))
            throw ApiError(DDPCA_EINVAL, "mcontact_gpu_stress: subdomain " + std::to_string(tv) + " is not owned by this rank");
        MULTIGRID& g = P.mc.multGrid[tv];
        if (g.elemVect.empty() || g.leveCount.empty() || g.numNodes() != g.nodalCount() || 3 * g.numNodes() != 3 * S.nn + S.nh)
            throw ApiError(DDPCA_EINVAL, "mcontact_gpu_stress: subdomain " + std::to_string(tv) +
                                             " has no element tree (an operator-level problem carries no mesh)");
        n = 7 * g.numNodes();
        if (!out) return;
        select_device(S.device);
        try {
            const double* d = stress_device(g, S.device, S.u_main, S.u_hang, S.nn, S.stream);
            DDPCA_HIP(hipStreamSynchronize(S.stream));
            stress_kernel_ms(g, last_kernel_ms);
            if (cap > 0) {
                SyncCallGuard guard;
                DDPCA_HIP(hipMemcpy(out, d, (size_t)std::min(n, cap) * sizeof(double), hipMemcpyDeviceToHost));
            }
        } catch (const std::invalid_argument& e) {
            throw ApiError(DDPCA_EINVAL, e.what());
        }
    });
    return rc < 0 ? rc : n;
}

}  // extern "C"
