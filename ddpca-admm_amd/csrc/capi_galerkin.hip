// C ABI of the Galerkin products (the chain of MULTIGRID::CONSTRAINT, MULTIGRID.h:1182-1184):
// ddpca_galerkin_rap on operands of the caller (k_rap on the device, or the host's galerkin_rap for
// device < 0), ddpca_multigrid_build_with and ddpca_problem_set_galerkin_device, which hand the chain
// of a build / of MCONTACT::ESTABLISH (MCONTACT.h:812-825) to the device.
#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/ddpca_amd.h"
#include "device_common.hpp"
#include "device_galerkin.hpp"
#include "device_stif.hpp"
#include "problem.hpp"

using namespace ddpca;

struct ddpca_galerkin {
    Bsr3 C;
};

namespace {

// of the calling thread's last device chain: pattern build, uploads (host clock), kernels (HIP
// events, summed over the levels), copies back (host clock); then each product's kernel time
thread_local double last_ms[4] = {0.0, 0.0, 0.0, 0.0};
thread_local std::vector<double> last_level_ms;

void run_chain(int device, const Bsr3& K, const std::vector<const Stencil*>& chain, std::vector<Bsr3>& out) {
    select_device(device);
    galerkin_chain_device(device, K, chain, out, last_ms, &last_level_ms);
}

// the Galerkin chain of CONSTRAINT on `device`, as MULTIGRID::galerkinChain takes it
GalerkinChain device_chain(int device) {
    return [device](const Bsr3& K, const std::vector<const Stencil*>& chain, std::vector<Bsr3>& out) {
        run_chain(device, K, chain, out);
    };
}

// n + 1 row pointers from 0, never decreasing
void check_ptr(const int64_t* ptr, int64_t n, const char* who) {
    if (ptr[0] != 0) throw ApiError(DDPCA_EINVAL, std::string(who) + ": row pointers do not start at 0");
    for (int64_t i = 0; i < n; ++i)
        if (ptr[i + 1] < ptr[i]) throw ApiError(DDPCA_EINVAL, std::string(who) + ": row pointers decrease");
}

}  // namespace

extern "C" {

// MULTIGRID.h:1182-1184
int ddpca_galerkin_rap(int device, int64_t nf, int64_t nc, const int64_t* a_ptr, const int32_t* a_col, const double* a_val,
                       const int64_t* s_ptr, const int32_t* s_col, const double* s_w, int64_t nbent, const int64_t* bent,
                       const double* bval, ddpca_galerkin_t* out) {
    return guarded([&] {
        if (!a_ptr || !a_col || !a_val || !s_ptr || !s_col || !s_w || !out || (nbent > 0 && (!bent || !bval)))
            throw ApiError(DDPCA_EINVAL, "ddpca_galerkin_rap: null argument");
        if (nf < 0 || nc < 0 || nbent < 0) throw ApiError(DDPCA_EINVAL, "ddpca_galerkin_rap: negative size");
        check_ptr(a_ptr, nf, "ddpca_galerkin_rap: A");
        check_ptr(s_ptr, nf, "ddpca_galerkin_rap: S");
        Bsr3 A;
        A.nb = A.mb = nf;
        A.ptr.assign(a_ptr, a_ptr + nf + 1);
        A.col.assign(a_col, a_col + a_ptr[nf]);
        for (int32_t c : A.col)
            if (c < 0 || c >= nf) throw ApiError(DDPCA_EINVAL, "ddpca_galerkin_rap: A is not nf x nf (column out of range)");
        A.val.assign(a_val, a_val + 9 * a_ptr[nf]);
        for (int64_t k = 0; k < s_ptr[nf]; ++k)
            if (s_col[k] < 0 || s_col[k] >= nc) throw ApiError(DDPCA_EINVAL, "ddpca_galerkin_rap: stencil column out of range");
        Stencil S = make_stencil(nf, nc, s_ptr, s_col, s_w);
        for (int64_t q = 0; q < nbent; ++q) {
            if (bent[q] < 0 || bent[q] >= s_ptr[nf]) throw ApiError(DDPCA_EINVAL, "ddpca_galerkin_rap: block entry out of range");
            if (q && bent[q] <= bent[q - 1]) throw ApiError(DDPCA_EINVAL, "ddpca_galerkin_rap: block entries not ascending");
        }
        S.bent.assign(bent, bent + nbent);
        S.bval.assign(bval, bval + 9 * nbent);
        auto h = std::make_unique<ddpca_galerkin>();
        if (device < 0) {
            h->C = galerkin_rap(A, S);
        } else {
            std::vector<Bsr3> lev;
            run_chain(device, A, {&S}, lev);
            h->C = std::move(lev[0]);
        }
        *out = h.release();
    });
}

// MULTIGRID.h:1182-1184
int ddpca_galerkin_view(ddpca_galerkin_t h, const int64_t** ptr, const int32_t** col, const double** val, int64_t* nb) {
    return guarded([&] {
        if (!h || !ptr || !col || !val || !nb) throw ApiError(DDPCA_EINVAL, "ddpca_galerkin_view: null argument");
        *ptr = h->C.ptr.data();
        *col = h->C.col.data();
        *val = h->C.val.data();
        *nb = h->C.nb;
    });
}

// MULTIGRID.h:1182-1184
int ddpca_galerkin_destroy(ddpca_galerkin_t h) {
    return guarded([&] { delete h; });
}

// MULTIGRID.h:722-1255 (ddpca_multigrid_build) with the element loop of 950-1039 and / or the
// Galerkin chain of 1182-1184 on the device
int ddpca_multigrid_build_with(ddpca_multigrid_t h, const ddpca_csr_t* extra, int assembly_device, int galerkin_device) {
    return guarded([&] {
        std::function<void(MULTIGRID&, double*)> values;
        GalerkinChain chain;
        if (galerkin_device >= 0) {
            select_device(galerkin_device);
            chain = device_chain(galerkin_device);
        }
        if (assembly_device >= 0) {
            select_device(assembly_device);
            values = stif_device_values(assembly_device);
        }
        multigrid_build(h, extra, values ? &values : nullptr, chain ? &chain : nullptr);
    });
}

// MCONTACT.h:812-825, MULTIGRID.h:1182-1184
int ddpca_problem_set_galerkin_device(ddpca_problem_t p, int device) {
    return guarded([&] {
        if (!p) throw ApiError(DDPCA_EINVAL, "ddpca_problem_set_galerkin_device: null problem");
        Problem& P = *reinterpret_cast<Problem*>(p);
        if (P.established) throw ApiError(DDPCA_ESTATE, "ddpca_problem_set_galerkin_device: problem already established");
        if (device < 0) {
            P.mc.galerkinBy = nullptr;
            return;
        }
        select_device(device);
        P.mc.galerkinBy = device_chain(device);
    });
}

// MULTIGRID.h:1182-1184 (measurement only)
int ddpca_galerkin_last_ms(double* out4) {
    return guarded([&] {
        if (!out4) throw ApiError(DDPCA_EINVAL, "ddpca_galerkin_last_ms: null argument");
        std::copy(last_ms, last_ms + 4, out4);
    });
}

int ddpca_galerkin_last_level_ms(double* out, int64_t cap) {
    if (!out || cap < 0) {
        set_last_error("ddpca_galerkin_last_level_ms: null argument");
        return DDPCA_EINVAL;
    }
    const int64_t n = std::min<int64_t>(cap, (int64_t)last_level_ms.size());
    std::copy(last_level_ms.begin(), last_level_ms.begin() + n, out);
    return (int)n;
}

}  // extern "C"
