// C ABI of the stiffness assembly (MULTIGRID::STIF_MATR, MULTIGRID.h:950-1039, and
// MULTIGRID::GET_VOLUME, MULTIGRID.h:1041-1082): ddpca_multigrid_stif / _volume on a built element
// tree (device kernels, or the host element loop for device < 0), ddpca_multigrid_build_on and
// ddpca_problem_set_assembly_device, which hand the element loop of a build / of
// MCONTACT::ESTABLISH (MCONTACT.h:812-825) to the device.
#include <chrono>

#include "../../include/ddpca_amd.h"
#include "device_common.hpp"
#include "device_stif.hpp"
#include "device_stress.hpp"
#include "problem.hpp"

using namespace ddpca;

namespace {

// of the calling thread's last device assembly: k_stif_elem, k_stif_gather (HIP events), then the
// host clock of the plan build, the upload (both 0 when cached) and the copy back
thread_local double last_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
// g's plan, built now if it has none; the host clock of that (0 when cached)
double plan_ms(MULTIGRID& g) {
    if (g.stifPlan) return 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    g.STIF_PLAN();
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the values of g's stiffness from `device`; built_ms: what the caller's plan_ms(g) returned
void run_device(MULTIGRID& g, int device, double* val, double built_ms) {
    select_device(device);
    double ms[4];
    stif_device(g, device, val, nullptr, ms);
    last_ms[0] = ms[0], last_ms[1] = ms[1], last_ms[2] = built_ms, last_ms[3] = ms[2], last_ms[4] = ms[3];
}

// the element loop of STIF_MATR on `device`, as STIF_MATR_BY takes it
std::function<void(MULTIGRID&, double*)> device_values(int device) {
    return [device](MULTIGRID& g, double* val) { run_device(g, device, val, plan_ms(g)); };
}

MULTIGRID& built_tree(ddpca_multigrid_t h, bool args_ok, const char* who) {
    bool built = false;
    MULTIGRID* g = multigrid_of(h, &built);
    if (!g || !args_ok) throw ApiError(DDPCA_EINVAL, std::string(who) + ": null argument");
    if (!built) throw ApiError(DDPCA_EINVAL, std::string(who) + ": ddpca_multigrid_build has not run");
    return *g;
}

}  // namespace

namespace ddpca {
std::function<void(MULTIGRID&, double* val)> stif_device_values(int device) { return device_values(device); }
}  // namespace ddpca

extern "C" {

int ddpca_stif_last_kernel_ms(double* out2) {
    return guarded([&] {
        if (!out2) throw ApiError(DDPCA_EINVAL, "ddpca_stif_last_kernel_ms: null argument");
        out2[0] = last_ms[0];
        out2[1] = last_ms[1];
    });
}

int ddpca_stif_last_host_ms(double* out3) {
    return guarded([&] {
        if (!out3) throw ApiError(DDPCA_EINVAL, "ddpca_stif_last_host_ms: null argument");
        for (int k = 0; k < 3; ++k) out3[k] = last_ms[2 + k];
    });
}

// MULTIGRID.h:950-1039
int ddpca_multigrid_stif(ddpca_multigrid_t h, int device, const int64_t** ptr, const int32_t** col, const double** val,
                         int64_t* nb) {
    return guarded([&] {
        MULTIGRID& g = built_tree(h, ptr && col && val && nb, "ddpca_multigrid_stif");
        try {
            if (device >= 0) select_device(device);
            const double built_ms = plan_ms(g);
            Bsr3& K = g.stifPlan->K;
            if (device < 0) {
                K.val.assign((size_t)9 * K.nnzb(), 0.0);
                g.STIF_VALUES(g.STIF_COLOURS(), K);
            } else {
                K.val.resize((size_t)9 * K.nnzb());  // every stored block is written by the gather
                run_device(g, device, K.val.data(), built_ms);
            }
            *ptr = K.ptr.data();
            *col = K.col.data();
            *val = K.val.data();
            *nb = K.nb;
        } catch (const std::invalid_argument& e) {
            throw ApiError(DDPCA_EINVAL, e.what());
        }
    });
}

// MULTIGRID.h:1041-1082
int ddpca_multigrid_volume(ddpca_multigrid_t h, int device, double* volume) {
    return guarded([&] {
        MULTIGRID& g = built_tree(h, volume != nullptr, "ddpca_multigrid_volume");
        try {
            if (device < 0) {
                *volume = g.GET_VOLUME();
                return;
            }
            select_device(device);
            *volume = volume_device(g, device);
        } catch (const std::invalid_argument& e) {
            throw ApiError(DDPCA_EINVAL, e.what());
        }
    });
}

// MULTIGRID.h:722-1255 (ddpca_multigrid_build) with the element loop of 950-1039 on the device
int ddpca_multigrid_build_on(ddpca_multigrid_t h, const ddpca_csr_t* extra, int device) {
    return guarded([&] {
        if (device < 0) {
            multigrid_build(h, extra, nullptr);
            return;
        }
        select_device(device);
        const auto values = device_values(device);
        multigrid_build(h, extra, &values);
    });
}

// MCONTACT.h:812-825
int ddpca_problem_set_assembly_device(ddpca_problem_t p, int device) {
    return guarded([&] {
        if (!p) throw ApiError(DDPCA_EINVAL, "ddpca_problem_set_assembly_device: null problem");
        Problem& P = *reinterpret_cast<Problem*>(p);
        if (P.established) throw ApiError(DDPCA_ESTATE, "ddpca_problem_set_assembly_device: problem already established");
        if (device < 0) {
            P.mc.stifValues = nullptr;
            return;
        }
        select_device(device);
        P.mc.stifValues = device_values(device);
    });
}

}  // extern "C"
