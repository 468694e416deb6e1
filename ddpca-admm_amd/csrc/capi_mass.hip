// C ABI of the batched surface-mass solver on its own: ddpca_mass_solve (include/ddpca_amd.h).
#include <algorithm>
#include <cstring>

#include "../../include/ddpca_amd.h"
#include "device_mass.hpp"

using namespace ddpca;

extern "C" {

int ddpca_mass_solve(int device, int64_t nsys, const ddpca_csr_t* A, const double* b, double* x, double rtol,
                     int64_t maxit, int fuse_alpha, int64_t* iters) {
    int64_t nrow = 0;
    std::vector<int64_t> roff;
    std::vector<Csr> store;         // one copy per distinct system
    std::vector<const Csr*> sys;    // system s -> its copy
    DevBuf<double> xd;
    MassBatch mb;
    hipStream_t st = nullptr;
    auto copy_out = [&]() {  // the systems' rows of the padded batch vector, in order
        std::vector<double> h(std::max<int64_t>(nrow, 1));
        DDPCA_HIP(hipMemcpy(h.data(), xd.p, nrow * sizeof(double), hipMemcpyDeviceToHost));
        int64_t o = 0;
        for (int64_t s = 0; s < nsys; ++s) {
            std::memcpy(x + o, h.data() + roff[s], sys[s]->nrow * sizeof(double));
            o += sys[s]->nrow;
        }
    };
    const int rc = guarded([&] {
        if (nsys < 1 || !A || !b || !x || !(rtol > 0.0) || maxit < 1) throw ApiError(DDPCA_EINVAL, "ddpca_mass_solve: arguments");
        select_device(device);
        store.reserve(nsys);  // sys points into it
        for (int64_t s = 0; s < nsys; ++s) {
            const ddpca_csr_t& a = A[s];
            // system s - nsys/2 handed over again (the same arrays): one Csr for both, so that
            // MassBatch::build sees the pair as the ADMM loop's fused w|v batch shows it
            const int64_t t = nsys % 2 == 0 && s >= nsys / 2 ? s - nsys / 2 : -1;
            if (t >= 0 && a.nrow == A[t].nrow && a.ncol == A[t].ncol && a.ptr == A[t].ptr && a.col == A[t].col &&
                a.val == A[t].val) {
                roff.push_back(nrow);
                nrow += pad64(a.nrow);
                sys.push_back(sys[t]);
                continue;
            }
            if (a.nrow < 1 || a.ncol != a.nrow || !a.ptr || (a.ptr[a.nrow] > 0 && (!a.col || !a.val)))
                throw ApiError(DDPCA_EINVAL, "ddpca_mass_solve: system " + std::to_string(s) + " is not a square CSR");
            Csr c;
            c.nrow = c.ncol = a.nrow;
            c.ptr.assign(a.ptr, a.ptr + a.nrow + 1);
            if (c.ptr[0] != 0) throw ApiError(DDPCA_EINVAL, "ddpca_mass_solve: ptr[0] != 0");
            for (int64_t r = 0; r < a.nrow; ++r)
                if (c.ptr[r + 1] < c.ptr[r]) throw ApiError(DDPCA_EINVAL, "ddpca_mass_solve: row pointer decreases");
            c.col.assign(a.col, a.col + c.ptr[a.nrow]);
            c.val.assign(a.val, a.val + c.ptr[a.nrow]);
            bool diag = false;
            for (int64_t r = 0; r < a.nrow; ++r)
                for (int64_t k = c.ptr[r]; k < c.ptr[r + 1]; ++k) {
                    if (c.col[k] < 0 || c.col[k] >= a.nrow) throw ApiError(DDPCA_EINVAL, "ddpca_mass_solve: column out of range");
                    diag |= c.col[k] == r;
                }
            if (!diag) throw ApiError(DDPCA_EINVAL, "ddpca_mass_solve: a system without diagonal entries");
            roff.push_back(nrow);
            nrow += pad64(a.nrow);
            store.push_back(std::move(c));
            sys.push_back(&store.back());
        }
        mb.build(sys, roff, nrow);
        mb.fuse_override = fuse_alpha;
        std::vector<double> hb(nrow, 0.0);
        int64_t o = 0;
        for (int64_t s = 0; s < nsys; ++s) {
            std::memcpy(hb.data() + roff[s], b + o, sys[s]->nrow * sizeof(double));
            o += sys[s]->nrow;
        }
        DDPCA_HIP(hipMemcpy(mb.b.p, hb.data(), nrow * sizeof(double), hipMemcpyHostToDevice));
        xd.alloc(nrow);
        DDPCA_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        mb.solve(st, xd.p, rtol, maxit);
        DDPCA_HIP(hipStreamSynchronize(st));
        if (iters)
            for (int64_t s = 0; s < nsys; ++s) iters[s] = mb.mirror.host[s].iter;
        copy_out();
        mb.check();  // DDPCA_ENUMERIC on a breakdown (x already copied: the last good iterate)
    });
    if (st) {
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
    }
    return rc;
}

}  // extern "C"
