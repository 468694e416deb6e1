// Contact search on the device (gfx950, fp64 throughout): the face pairs of CSEARCH::CONTACT_SEARCH /
// SEGMENT_INTERSECT (CSEARCH.h:614-817) from the host's plan (csearch.cpp, csearch_plan: bucket sort,
// candidate pairs in the reference's order), with the arithmetic of csearch_face.hpp -- the same
// operations in the same order as the host search, compiled without contraction.
//
//   k_cs_count   one thread per candidate (slave face, master face) pair, 64 pairs per workgroup.
//                The thread projects the four slave corners onto the master face, clips the two
//                quads, orders the polygon and walks its quadrature points until one has
//                gap <= maxiDist; it stores the pair's point count (4 per polygon vertex) or 0.
//                The clip list, the polygon and the vertex angles (3 x 40 doubles, runtime-indexed)
//                are the thread's columns of an LDS array (element i of lane l at [64 i + l]: no
//                bank conflict among the lanes of a wavefront, no barrier: a column is private).
//   scan         the counts are copied back and scanned on the host (int64 offsets, the kept pairs
//                compacted in pair order): deterministic, no atomics.
//   k_cs_emit    one thread per kept pair: the polygon again, then every quadrature point written at
//                the pair's offset straight into ddpca_ips_get's layout (kValues = false: the node
//                ids only, for ddpca_refine_select_on, and no projection of the points).
// No loop without a bound: Newton loops 60, PROJECT_STM's stepped approach `cap` (csearch_plan
// refuses input whose cap would pass 2^20).  Every index is checked against the pair / kept count
// before any load.  Resource usage and measurement: DESIGN.md "Contact search".
#include "device_csearch.hpp"

#include <chrono>

#include "csearch_face.hpp"
#include "device_common.hpp"

namespace ddpca {

namespace {

constexpr int kPairBlock = 64;  // pairs (threads) per workgroup: 3 * 40 * 64 doubles = 60 KiB of LDS

struct PairLds {
    double v[3 * csface::kMaxClip * kPairBlock];
};

__device__ __forceinline__ csface::Slots lane_slots(PairLds& L) {
    double* b = L.v + threadIdx.x;
    return csface::Slots{b, b + csface::kMaxClip * kPairBlock, b + 2 * csface::kMaxClip * kPairBlock, kPairBlock};
}

__device__ __forceinline__ void load_corners(const double* __restrict__ xyz, const int32_t* __restrict__ seg,
                                             double (&c)[4][3], int32_t (&nd)[4]) {
    const int4 s = *reinterpret_cast<const int4*>(seg);
    nd[0] = s.x, nd[1] = s.y, nd[2] = s.z, nd[3] = s.w;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) c[k][a] = xyz[3 * (int64_t)nd[k] + a];
}

__global__ __launch_bounds__(kPairBlock) void k_cs_count(int64_t npair, const int32_t* __restrict__ pair_slav,
                                                         const int32_t* __restrict__ pair_mast,
                                                         const double* __restrict__ mast_xyz,
                                                         const double* __restrict__ slav_xyz,
                                                         const int32_t* __restrict__ mast_face,
                                                         const int32_t* __restrict__ slav_face, long cap, double maxiDist,
                                                         int32_t* __restrict__ count) {
    __shared__ PairLds lds;
    const int64_t p = (int64_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (p >= npair) return;  // nothing below crosses lanes
    double mc[4][3], sc[4][3], cx, cy;
    int32_t mn[4], sn[4];
    load_corners(mast_xyz, mast_face + 4 * (int64_t)pair_mast[p], mc, mn);
    load_corners(slav_xyz, slav_face + 4 * (int64_t)pair_slav[p], sc, sn);
    count[p] = csface::pair_count(mc, sc, cap, maxiDist, lane_slots(lds), cx, cy);
}

template <bool kValues>
__global__ __launch_bounds__(kPairBlock) void k_cs_emit(int64_t nkept, int64_t npoint, const int32_t* __restrict__ kept,
                                                        const int64_t* __restrict__ off,
                                                        const int32_t* __restrict__ pair_slav,
                                                        const int32_t* __restrict__ pair_mast,
                                                        const double* __restrict__ mast_xyz,
                                                        const double* __restrict__ slav_xyz,
                                                        const int32_t* __restrict__ mast_face,
                                                        const int32_t* __restrict__ slav_face, long cap,
                                                        int64_t* __restrict__ node, double* __restrict__ shap,
                                                        double* __restrict__ basis, double* __restrict__ gap,
                                                        double* __restrict__ w) {
    __shared__ PairLds lds;
    const int64_t e = (int64_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (e >= nkept) return;
    const int64_t p = kept[e];
    double mc[4][3], sc[4][3], g[4][3], cx, cy;
    int32_t mn[4], sn[4];
    load_corners(mast_xyz, mast_face + 4 * (int64_t)pair_mast[p], mc, mn);
    load_corners(slav_xyz, slav_face + 4 * (int64_t)pair_slav[p], sc, sn);
    const csface::Slots S = lane_slots(lds);
    const int n = csface::polygon(mc, sc, cap, S, cx, cy);
    // the count pass ran the same code on the same input: 4 n is what the scan reserved.  The end
    // of the pair's range is checked all the same, so that nothing can be written past the arrays
    const int64_t o0 = off[e], o1 = off[e + 1] < npoint ? off[e + 1] : npoint;
    if (kValues) csface::bilinear(sc, g);
#pragma unroll 1
    for (int q = 0; q < 4 * n; ++q) {
        const int64_t o = o0 + q;
        if (o >= o1) break;
#pragma unroll
        for (int k = 0; k < 4; ++k) node[8 * o + k] = mn[k], node[8 * o + 4 + k] = sn[k];
        if (kValues) {
            double px, py, wq;
            csface::quad_point(S, n, cx, cy, q, px, py, wq);
            csface::Point pt;
            csface::point(mc, sc, g, px, py, wq, pt);
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int k = 0; k < 4; ++k) shap[8 * o + 4 * s + k] = pt.shap[s][k];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) basis[9 * o + 3 * a + b] = pt.basis[a][b];
            gap[o] = pt.gap;
            w[o] = pt.w;
        }
    }
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// a device allocation that names its size when it fails (no host fallback)
template <typename T>
void alloc_or_explain(DevBuf<T>& b, size_t count, const char* what) {
    try {
        b.alloc(count);
    } catch (const ApiError& e) {
        (void)hipGetLastError();
        throw ApiError(DDPCA_EHIP, std::string("contact search: ") + what + " needs " + std::to_string(count * sizeof(T)) +
                                       " bytes of device memory (" + e.what() + ")");
    }
}
template <typename T>
void upload_or_explain(DevBuf<T>& b, const T* h, size_t count, const char* what) {
    alloc_or_explain(b, count, what);
    if (count) {
        SyncCallGuard g;
        DDPCA_HIP(hipMemcpy(b.p, h, count * sizeof(T), hipMemcpyHostToDevice));
    }
}
template <typename T>
void copy_back(T* h, const DevBuf<T>& b, size_t count) {
    if (count) {
        SyncCallGuard g;
        DDPCA_HIP(hipMemcpy(h, b.p, count * sizeof(T), hipMemcpyDeviceToHost));
    }
}

struct Events {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    Events() {
        for (hipEvent_t& e : ev) DDPCA_HIP(hipEventCreate(&e));
    }
    ~Events() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    double ms(int a, int b) const {
        float t = 0.0f;
        DDPCA_HIP(hipEventElapsedTime(&t, ev[a], ev[b]));
        return t;
    }
};

}  // namespace

void csearch_device(const CsearchInput& in, const CsearchPlan& P, bool values, ddpca_ips& out, double ms[4],
                    int64_t pairs[3]) {
    const int64_t np = (int64_t)P.pair_slav.size();
    pairs[0] = np, pairs[1] = 0, pairs[2] = 0;
    ms[0] = ms[1] = ms[2] = ms[3] = 0.0;
    out = ddpca_ips{};
    if (np == 0) return;
    if (np >= (int64_t)1 << 31) throw ApiError(DDPCA_EINVAL, "contact search: 2^31 or more candidate pairs");
    auto t0 = std::chrono::steady_clock::now();
    DevBuf<double> mxyz, sxyz;
    DevBuf<int32_t> mface, sface, pslav, pmast, count;
    upload_or_explain(mxyz, in.mast_xyz, (size_t)3 * in.mast_nnode, "the master coordinates");
    upload_or_explain(sxyz, in.slav_xyz, (size_t)3 * in.slav_nnode, "the slave coordinates");
    upload_or_explain(mface, P.mast_face.data(), P.mast_face.size(), "the master faces");
    upload_or_explain(sface, P.slav_face.data(), P.slav_face.size(), "the slave faces");
    upload_or_explain(pslav, P.pair_slav.data(), (size_t)np, "the pair list (slave faces)");
    upload_or_explain(pmast, P.pair_mast.data(), (size_t)np, "the pair list (master faces)");
    alloc_or_explain(count, (size_t)np, "the pair counts");
    ms[0] = ms_since(t0);
    Events E;
    DDPCA_HIP(hipEventRecord(E.ev[0], nullptr));
    hipLaunchKernelGGL(k_cs_count, dim3((unsigned)((np + kPairBlock - 1) / kPairBlock)), dim3(kPairBlock), 0, nullptr, np,
                       pslav.p, pmast.p, mxyz.p, sxyz.p, mface.p, sface.p, P.cap, in.maxiDist, count.p);
    DDPCA_HIP(hipGetLastError());
    DDPCA_HIP(hipEventRecord(E.ev[1], nullptr));
    DDPCA_HIP(hipStreamSynchronize(nullptr));
    t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> hcount((size_t)np);
    copy_back(hcount.data(), count, (size_t)np);
    count.release();
    std::vector<int32_t> kept;
    std::vector<int64_t> off;
    int64_t total = 0;
    for (int64_t p = 0; p < np; ++p) {
        const int32_t c = hcount[p];
        if (c < 0 || c > csface::kMaxPoints) throw ApiError(DDPCA_EHIP, "contact search: a pair count outside 0 .. 160 came back");
        if (c > 0) {
            kept.push_back((int32_t)p);
            off.push_back(total);
            total += c;
        }
    }
    off.push_back(total);
    const int64_t nk = (int64_t)kept.size();
    ms[1] = E.ms(0, 1) + ms_since(t0);
    pairs[1] = nk, pairs[2] = total;
    if (nk == 0) return;
    t0 = std::chrono::steady_clock::now();
    DevBuf<int32_t> dkept;
    DevBuf<int64_t> doff, dnode;
    DevBuf<double> dshap, dbasis, dgap, dw;
    upload_or_explain(dkept, kept.data(), (size_t)nk, "the kept pairs");
    upload_or_explain(doff, off.data(), (size_t)nk + 1, "the point offsets");
    alloc_or_explain(dnode, (size_t)8 * total, "the points' node ids");
    if (values) {
        alloc_or_explain(dshap, (size_t)8 * total, "the points' shape values");
        alloc_or_explain(dbasis, (size_t)9 * total, "the points' bases");
        alloc_or_explain(dgap, (size_t)total, "the points' gaps");
        alloc_or_explain(dw, (size_t)total, "the points' weights");
    }
    ms[0] += ms_since(t0);
    const dim3 grid((unsigned)((nk + kPairBlock - 1) / kPairBlock));
    DDPCA_HIP(hipEventRecord(E.ev[2], nullptr));
    if (values)
        hipLaunchKernelGGL(k_cs_emit<true>, grid, dim3(kPairBlock), 0, nullptr, nk, total, dkept.p, doff.p, pslav.p, pmast.p,
                           mxyz.p, sxyz.p, mface.p, sface.p, P.cap, dnode.p, dshap.p, dbasis.p, dgap.p, dw.p);
    else
        hipLaunchKernelGGL(k_cs_emit<false>, grid, dim3(kPairBlock), 0, nullptr, nk, total, dkept.p, doff.p, pslav.p, pmast.p,
                           mxyz.p, sxyz.p, mface.p, sface.p, P.cap, dnode.p, nullptr, nullptr, nullptr, nullptr);
    DDPCA_HIP(hipGetLastError());
    DDPCA_HIP(hipEventRecord(E.ev[3], nullptr));
    DDPCA_HIP(hipStreamSynchronize(nullptr));
    ms[2] = E.ms(2, 3);
    t0 = std::chrono::steady_clock::now();
    out.resize(total, values);
    copy_back(out.node.get(), dnode, (size_t)8 * total);
    if (values) {
        copy_back(out.shap.get(), dshap, (size_t)8 * total);
        copy_back(out.basis.get(), dbasis, (size_t)9 * total);
        copy_back(out.gap.get(), dgap, (size_t)total);
        copy_back(out.w.get(), dw, (size_t)total);
    }
    ms[3] = ms_since(t0);
}

}  // namespace ddpca
