// Galerkin products on the device (gfx950, fp64 throughout): the chain of MULTIGRID::CONSTRAINT,
// MULTIGRID.h:1182-1184, C = P^T A P with P = S (x) I3 plus S's 3x3 block entries, on the pattern
// of galerkin_pattern (sparse.cpp; the pattern is the host's own).
//
//   k_rap<false>   one wavefront per coarse row c1, four rows per workgroup.  Lane j owns the stored
//                  block (c1, col[ptr[c1] + j]) with nine accumulators in registers; a row with more
//                  than 64 stored blocks takes further passes of 64 over the same traversal.  The
//                  wave walks, wave-uniformly and in galerkin_rap's order, the children f1 of c1
//                  (ascending), the blocks k of A's row f1 (as stored), the entries s of S's row f2;
//                  the lane whose column is S.col[s] adds (w1 w2) A_k, one fma per component.  A
//                  gather with one owner per block: no atomics, no LDS, bit-identical run to run,
//                  nothing depends on where a workgroup runs.  Every loop is bounded by the CSR
//                  pointers of the operands, which the entry points check before the launch.
//   k_rap<true>    the same walk for a stencil with block entries (rotated nodes): T = B1^T A_k per
//                  block of A, then acc += T B2 in the owning lane, a scalar entry read as w I: the
//                  arithmetic of galerkin_rap_blocks with each three-term sum as one fma chain.
// Byte model, resource usage and measurements: DESIGN.md §3e.
#include "device_galerkin.hpp"

#include <chrono>
#include <mutex>

#include "../../include/ddpca_amd.h"
#include "device_common.hpp"

namespace ddpca {

namespace {

constexpr int kRowsPerBlock = kBlock / kWave;

// the 3x3 block of stencil entry e: its block entry, or w I
__device__ __forceinline__ void entry_block(int64_t e, const double* __restrict__ sw, const int32_t* __restrict__ sblk,
                                            const double* __restrict__ bval, double B[9]) {
    const int32_t q = sblk[e];
    if (q >= 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) B[i] = bval[9 * (int64_t)q + i];
    } else {
        const double w = sw[e];
#pragma unroll
        for (int i = 0; i < 9; ++i) B[i] = i % 4 == 0 ? w : 0.0;
    }
}

template <bool kBlocks>
__global__ __launch_bounds__(kBlock) void k_rap(int64_t nc, const int64_t* __restrict__ cptr, const int32_t* __restrict__ ccol,
                                                const int64_t* __restrict__ tptr, const int32_t* __restrict__ tfine,
                                                const int64_t* __restrict__ tent, const int64_t* __restrict__ aptr,
                                                const int32_t* __restrict__ acol, const double* __restrict__ aval,
                                                const int64_t* __restrict__ sptr, const int32_t* __restrict__ scol,
                                                const double* __restrict__ sw, const int32_t* __restrict__ sblk,
                                                const double* __restrict__ bval, double* __restrict__ cval) {
    const int lane = threadIdx.x & (kWave - 1);
    // the row is the same in every lane of the wave: say so, the walk below is scalar then
    const int64_t c1 = (int64_t)blockIdx.x * kRowsPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    if (c1 >= nc) return;
    const int64_t r0 = cptr[c1], r1 = cptr[c1 + 1];
    const int64_t t0 = tptr[c1], t1 = tptr[c1 + 1];
    for (int64_t base = r0; base < r1; base += kWave) {
        const int64_t mine = base + lane;
        const bool have = mine < r1;
        const int32_t mycol = have ? ccol[mine] : -1;  // no stencil column is negative
        double acc[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) acc[q] = 0.0;
        for (int64_t t = t0; t < t1; ++t) {
            const int64_t f1 = tfine[t];
            const int64_t e1 = tent[t];
            double w1 = 0.0;
            double B1[9];
            if constexpr (kBlocks) entry_block(e1, sw, sblk, bval, B1);
            else w1 = sw[e1];
            for (int64_t k = aptr[f1]; k < aptr[f1 + 1]; ++k) {
                const int64_t f2 = acol[k];
                double a[9];
#pragma unroll
                for (int q = 0; q < 9; ++q) a[q] = aval[9 * k + q];
                double T[9];  // B1^T A_k
                if constexpr (kBlocks) {
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j)
                            T[3 * i + j] = fma(B1[6 + i], a[6 + j], fma(B1[3 + i], a[3 + j], B1[i] * a[j]));
                }
                for (int64_t s = sptr[f2]; s < sptr[f2 + 1]; ++s) {
                    if (scol[s] != mycol) continue;
                    if constexpr (kBlocks) {
                        double B2[9];
                        entry_block(s, sw, sblk, bval, B2);
#pragma unroll
                        for (int i = 0; i < 3; ++i)
#pragma unroll
                            for (int j = 0; j < 3; ++j)
                                acc[3 * i + j] += fma(T[3 * i + 2], B2[6 + j], fma(T[3 * i + 1], B2[3 + j], T[3 * i] * B2[j]));
                    } else {
                        const double ww = w1 * sw[s];
#pragma unroll
                        for (int q = 0; q < 9; ++q) acc[q] = fma(ww, a[q], acc[q]);
                    }
                }
            }
        }
        if (have) {
#pragma unroll
            for (int q = 0; q < 9; ++q) cval[9 * mine + q] = acc[q];
        }
    }
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// an upload whose failure names what was being uploaded and its size
template <typename T>
void upload_or_explain(DevBuf<T>& b, const T* h, size_t count, const char* what) {
    try {
        b.upload(h, count);
    } catch (const ApiError& e) {
        (void)hipGetLastError();
        throw ApiError(e.code, std::string("Galerkin product: ") + what + " needs " + std::to_string(count * sizeof(T)) +
                                   " bytes of device memory (" + e.what() + ")");
    }
}
template <typename T>
void upload_or_explain(DevBuf<T>& b, const std::vector<T>& v, const char* what) {
    upload_or_explain(b, v.data(), v.size(), what);
}

struct Events {
    hipEvent_t ev[2] = {nullptr, nullptr};
    Events() {
        for (hipEvent_t& e : ev) DDPCA_HIP(hipEventCreate(&e));
    }
    ~Events() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    Events(const Events&) = delete;
    Events& operator=(const Events&) = delete;
};

void check_int32(int64_t n, const char* what) {
    if (n >= (int64_t(1) << 31)) throw ApiError(DDPCA_EINVAL, std::string("Galerkin product: ") + what + " does not fit int32 indices");
}

// one chain at a time on the GPU: the host threads of ESTABLISH's loop queue here
std::mutex& chain_mutex() {
    static std::mutex m;
    return m;
}

}  // namespace

void galerkin_chain_device(int device, const Bsr3& K, const std::vector<const Stencil*>& chain, std::vector<Bsr3>& out,
                           double ms[4], std::vector<double>* level_ms) {
    (void)device;  // current already (select_device by the caller)
    const size_t nlev = chain.size();
    double t_pattern = 0.0, t_upload = 0.0, t_kernel = 0.0, t_back = 0.0;
    if (level_ms) level_ms->assign(nlev, 0.0);
    // ---- the patterns, on the host, before the GPU is taken
    auto t0 = std::chrono::steady_clock::now();
    out.assign(nlev, Bsr3());
    std::vector<GalerkinPattern> pat(nlev);
    check_int32(K.nnzb(), "the finest operator");
    for (size_t i = 0; i < nlev; ++i) {
        const Bsr3& A = i ? out[i - 1] : K;
        const Stencil& S = *chain[i];
        if (S.nf != A.nb || A.nb != A.mb) throw ApiError(DDPCA_EINVAL, "Galerkin product: the stencil's rows are not the operator's nodes");
        check_int32((int64_t)S.col.size(), "the stencil");
        pat[i] = galerkin_pattern(A, S);
        check_int32((int64_t)pat[i].col.size(), "the product");
        out[i].nb = out[i].mb = S.nc;
        out[i].ptr = std::move(pat[i].ptr);
        out[i].col = std::move(pat[i].col);
    }
    t_pattern = ms_since(t0);
    // the host arrays the values come back into: sized (and their pages touched) here, not while
    // the GPU is held; counted with the copies back
    t0 = std::chrono::steady_clock::now();
    for (Bsr3& C : out) C.val.resize((size_t)9 * C.col.size());
    t_back = ms_since(t0);

    std::lock_guard<std::mutex> gpu(chain_mutex());
    Events E;
    // ---- the finest operator, once
    t0 = std::chrono::steady_clock::now();
    DevBuf<int64_t> aptr;
    DevBuf<int32_t> acol;
    DevBuf<double> aval;
    if (nlev) {
        upload_or_explain(aptr, K.ptr, "the finest operator's row pointers");
        upload_or_explain(acol, K.col, "the finest operator's columns");
        upload_or_explain(aval, K.val, "the finest operator's blocks");
    }
    t_upload += ms_since(t0);
    for (size_t i = 0; i < nlev; ++i) {
        const Stencil& S = *chain[i];
        Bsr3& C = out[i];
        const bool blocks = !S.bent.empty();
        t0 = std::chrono::steady_clock::now();
        DevBuf<int64_t> cptr, tptr, tent, sptr;
        DevBuf<int32_t> ccol, tfine, scol, sblk;
        DevBuf<double> sw, bval, cval;
        upload_or_explain(cptr, C.ptr, "the product's row pointers");
        upload_or_explain(ccol, C.col, "the product's columns");
        upload_or_explain(tptr, pat[i].tptr, "the stencil's transpose");
        upload_or_explain(tfine, pat[i].tfine, "the stencil's transpose");
        upload_or_explain(tent, pat[i].tent, "the stencil's transpose");
        upload_or_explain(sptr, S.ptr, "the stencil");
        upload_or_explain(scol, S.col, "the stencil");
        upload_or_explain(sw, S.w, "the stencil");
        if (blocks) {
            std::vector<int32_t> blk_of(S.col.size(), -1);
            for (size_t q = 0; q < S.bent.size(); ++q) blk_of[S.bent[q]] = (int32_t)q;
            upload_or_explain(sblk, blk_of, "the stencil's block index");
            upload_or_explain(bval, S.bval, "the stencil's blocks");
        }
        try {
            cval.alloc((size_t)9 * C.col.size());
        } catch (const ApiError& e) {
            (void)hipGetLastError();
            throw ApiError(e.code, "Galerkin product: the product's blocks need " + std::to_string(9 * C.col.size() * sizeof(double)) +
                                       " bytes of device memory (" + e.what() + ")");
        }
        t_upload += ms_since(t0);
        if (S.nc > 0) {
            const dim3 grid((unsigned)ceil_div(S.nc, kRowsPerBlock)), block(kBlock);
            DDPCA_HIP(hipEventRecord(E.ev[0], nullptr));
            if (blocks)
                hipLaunchKernelGGL(k_rap<true>, grid, block, 0, nullptr, S.nc, cptr.p, ccol.p, tptr.p, tfine.p, tent.p, aptr.p,
                                   acol.p, aval.p, sptr.p, scol.p, sw.p, sblk.p, bval.p, cval.p);
            else
                hipLaunchKernelGGL(k_rap<false>, grid, block, 0, nullptr, S.nc, cptr.p, ccol.p, tptr.p, tfine.p, tent.p, aptr.p,
                                   acol.p, aval.p, sptr.p, scol.p, sw.p, (const int32_t*)nullptr, (const double*)nullptr, cval.p);
            DDPCA_HIP(hipGetLastError());
            DDPCA_HIP(hipEventRecord(E.ev[1], nullptr));
        }
        // ---- the copy back (synchronises the stream)
        t0 = std::chrono::steady_clock::now();
        if (!C.val.empty()) {
            SyncCallGuard g;
            DDPCA_HIP(hipMemcpy(C.val.data(), cval.p, C.val.size() * sizeof(double), hipMemcpyDeviceToHost));
        }
        DDPCA_HIP(hipStreamSynchronize(nullptr));
        t_back += ms_since(t0);
        if (S.nc > 0) {
            float e = 0.0f;
            DDPCA_HIP(hipEventElapsedTime(&e, E.ev[0], E.ev[1]));
            t_kernel += e;
            if (level_ms) (*level_ms)[i] = e;
        }
        // the product is the next level's operator; the finer level's device copy goes here
        aptr = std::move(cptr);
        acol = std::move(ccol);
        aval = std::move(cval);
    }
    if (ms) ms[0] = t_pattern, ms[1] = t_upload, ms[2] = t_kernel, ms[3] = t_back;
}

}  // namespace ddpca
