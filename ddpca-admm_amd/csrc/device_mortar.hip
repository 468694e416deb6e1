// The mortar operators of Interface::BUILD on the device (gfx950, fp64 throughout): the values of the
// nine operators of each interface side at the positions of the host's plan (mortar_plan.cpp), with
// the arithmetic of mortar_point.hpp -- the same operations in the same order as BUILD, compiled
// without contraction.  No atomics anywhere: every value has one writer, and every sum runs in one
// thread in the host's order.
//
//   k_mortar_pair<C>   one wavefront per contact node c, one lane per partner of c, in passes of 64
//                      when c has more.  Every lane walks c's incidence list in order (all lanes load
//                      the same point: a broadcast load) and, for each (q, a) and each b whose
//                      ipc[4 q + b] is the lane's partner, adds BUILD's terms into its registers:
//                      aGP and aG (9 + 9) for C = 3; aGP, aN and aM (9 + 3 + 1) for C = 1 (systMass
//                      needs aGP there too).
//   k_mortar_nodal<C>  one thread per stored pair: systMass (through bypos), systTran(_pena) (R^T
//                      applied where the row's node has a rotation), inteMass(_pena).
//   k_mortar_ip<C>     one thread per incidence-list position (its C x C values of inteInpo), then
//                      one thread per point (its rows of inpoLagr, inpoDisp -- columns rotated where
//                      needed -- and pemaInpo_r, through ord_c / ord_n).
// Every loop is bounded by a count of the view, every index is checked against it before a load and
// every write against the length of its operator (mortar::put).  Resource usage and measurement:
// DESIGN.md "Mortar operators".
#include "device_mortar.hpp"

#include <chrono>
#include <string>

#include "../../include/ddpca_amd.h"
#include "device_common.hpp"

namespace ddpca {

namespace {

using mortar::MortarView;

template <int C>
__global__ __launch_bounds__(kBlock) void k_mortar_pair(const MortarView V) {
    const int64_t c = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (c >= V.ncn) return;  // a whole wavefront; nothing below crosses lanes
    const int lane = threadIdx.x % kWave;
    const int32_t np = V.pptr[c + 1] - V.pptr[c];
#pragma unroll 1
    for (int32_t t0 = 0; t0 < np; t0 += kWave)
        if (t0 + lane < np) mortar::pair_lane<C>(V, (int32_t)c, t0 + lane);
}

template <int C>
__global__ __launch_bounds__(kBlock) void k_mortar_nodal(const MortarView V) {
    mortar::nodal_emit<C>(V, (int64_t)blockIdx.x * kBlock + threadIdx.x);  // checks k < npair itself
}

template <int C>
__global__ __launch_bounds__(kBlock) void k_mortar_ip(const MortarView V) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < V.ninc) mortar::inpo_emit<C>(V, i);
    else mortar::point_emit<C>(V, i - V.ninc);  // checks q < nip itself
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
        throw ApiError(DDPCA_EHIP, std::string("mortar operators: ") + what + " needs " + std::to_string(count * sizeof(T)) +
                                       " bytes of device memory (" + e.what() + ")");
    }
}
template <typename T>
const T* upload_or_explain(DevBuf<T>& b, const T* h, size_t count, const char* what) {
    alloc_or_explain(b, count, what);
    if (count) {
        SyncCallGuard g;
        DDPCA_HIP(hipMemcpy(b.p, h, count * sizeof(T), hipMemcpyHostToDevice));
    }
    return b.p;
}
template <typename T>
const T* upload_or_explain(DevBuf<T>& b, const std::vector<T>& v, const char* what) {
    return upload_or_explain(b, v.data(), v.size(), what);
}
void copy_back(std::vector<double>& h, const DevBuf<double>& b) {
    h.resize(b.n);
    if (b.n) {
        SyncCallGuard g;
        DDPCA_HIP(hipMemcpy(h.data(), b.p, b.n * sizeof(double), hipMemcpyDeviceToHost));
    }
}

struct Events {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
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

unsigned blocks_of(int64_t threads, int64_t per_block) {
    const int64_t b = (threads + per_block - 1) / per_block;
    if (b > INT32_MAX) throw ApiError(DDPCA_EINVAL, "mortar operators: more than 2^31 - 1 workgroups");
    return (unsigned)b;
}

template <int C>
void launch_side(const MortarView& V) {
    if (V.ncn > 0)
        hipLaunchKernelGGL(k_mortar_pair<C>, dim3(blocks_of(V.ncn, kBlock / kWave)), dim3(kBlock), 0, nullptr, V);
    DDPCA_HIP(hipGetLastError());
}
template <int C>
void launch_emit(const MortarView& V) {
    if (V.npair > 0) hipLaunchKernelGGL(k_mortar_nodal<C>, dim3(blocks_of(V.npair, kBlock)), dim3(kBlock), 0, nullptr, V);
    DDPCA_HIP(hipGetLastError());
    if (V.ninc + V.nip > 0)
        hipLaunchKernelGGL(k_mortar_ip<C>, dim3(blocks_of(V.ninc + V.nip, kBlock)), dim3(kBlock), 0, nullptr, V);
    DDPCA_HIP(hipGetLastError());
}

}  // namespace

void mortar_build_device(const MortarInput& in, Interface& itf, double ms[5]) {
    for (int k = 0; k < 5; ++k) ms[k] = 0.0;
    auto t0 = std::chrono::steady_clock::now();
    MortarPlan P = mortar_plan(in);  // refuses what the kernels' indices cannot hold, before any launch
    ms[0] = ms_since(t0);
    MortarValues val[2];
    t0 = std::chrono::steady_clock::now();
    DevBuf<double> pts;
    upload_or_explain(pts, reinterpret_cast<const double*>(in.ip), (size_t)mortar::kPointWords * in.nip, "the integration points");
    ms[1] += ms_since(t0);
    Events E;
    for (int s = 0; s < 2; ++s) {
        const MortarSide& S = P.side[s];
        MortarValues& v = val[s];
        t0 = std::chrono::steady_clock::now();
        MortarView V = S.view(s, in.C, in.penN, in.penF);
        V.pts = pts.p;
        DevBuf<int32_t> ipc, inc_ptr, inc, inc_node, pptr, part, pair_node, byrank, nrow0, rotidx;
        DevBuf<uint8_t> ord_c, ord_n;
        DevBuf<double> rot, aGP, aG, aN, aM, mass, tran, tranp, imass, imassp, lagr, disp, inpo, pema;
        V.ipc = upload_or_explain(ipc, S.ipc, "the points' contact indices");
        V.inc_ptr = upload_or_explain(inc_ptr, S.inc_ptr, "the incidence list's row pointers");
        V.inc = upload_or_explain(inc, S.inc, "the incidence list");
        V.inc_node = upload_or_explain(inc_node, S.inc_node, "the incidence list's nodes");
        V.pptr = upload_or_explain(pptr, S.pptr, "the partner lists' row pointers");
        V.part = upload_or_explain(part, S.part, "the partner lists");
        V.pair_node = upload_or_explain(pair_node, S.pair_node, "the pairs' contact nodes");
        V.byrank = upload_or_explain(byrank, S.byrank, "the pairs' systMass positions");
        V.nrow0 = upload_or_explain(nrow0, S.nrow0, "the contact nodes' row offsets");
        V.rotidx = upload_or_explain(rotidx, S.rotidx, "the contact nodes' rotation indices");
        V.ord_c = upload_or_explain(ord_c, S.ord_c, "the points' contact-index order");
        V.ord_n = upload_or_explain(ord_n, S.ord_n, "the points' node order");
        V.rot = upload_or_explain(rot, S.rot, "the rotations");
        alloc_or_explain(aGP, (size_t)9 * S.npair, "the pair sums (T^T P T)");
        V.aGP = aGP.p;
        if (in.C == 3) {
            alloc_or_explain(aG, (size_t)9 * S.npair, "the pair sums (T^T T)");
            V.aG = aG.p;
        } else {
            alloc_or_explain(aN, (size_t)3 * S.npair, "the pair sums (normal)");
            alloc_or_explain(aM, (size_t)S.npair, "the pair sums (mass)");
            V.aN = aN.p, V.aM = aM.p;
        }
        alloc_or_explain(mass, (size_t)V.n_mass, "systMass");
        alloc_or_explain(tran, (size_t)V.n_tran, "systTran");
        alloc_or_explain(tranp, (size_t)V.n_tran, "systTran_pena");
        alloc_or_explain(imass, (size_t)V.n_imass, "inteMass");
        alloc_or_explain(imassp, (size_t)V.n_imass, "inteMass_pena");
        alloc_or_explain(lagr, (size_t)V.n_lagr, "inpoLagr");
        alloc_or_explain(disp, (size_t)V.n_disp, "inpoDisp");
        alloc_or_explain(pema, (size_t)V.n_disp, "pemaInpo_r");
        alloc_or_explain(inpo, (size_t)V.n_inpo, "inteInpo");
        V.mass = mass.p, V.tran = tran.p, V.tranp = tranp.p, V.imass = imass.p, V.imassp = imassp.p;
        V.lagr = lagr.p, V.disp = disp.p, V.pema = pema.p, V.inpo = inpo.p;
        ms[1] += ms_since(t0);
        DDPCA_HIP(hipEventRecord(E.ev[0], nullptr));
        if (in.C == 3) launch_side<3>(V);
        else launch_side<1>(V);
        DDPCA_HIP(hipEventRecord(E.ev[1], nullptr));
        if (in.C == 3) launch_emit<3>(V);
        else launch_emit<1>(V);
        DDPCA_HIP(hipEventRecord(E.ev[2], nullptr));
        DDPCA_HIP(hipStreamSynchronize(nullptr));
        ms[2] += E.ms(0, 1);
        ms[3] += E.ms(1, 2);
        t0 = std::chrono::steady_clock::now();
        copy_back(v.mass, mass), copy_back(v.tran, tran), copy_back(v.tranp, tranp);
        copy_back(v.imass, imass), copy_back(v.imassp, imassp);
        copy_back(v.lagr, lagr), copy_back(v.disp, disp), copy_back(v.pema, pema), copy_back(v.inpo, inpo);
        ms[4] += ms_since(t0);
    }
    mortar_finish(in, P, val, itf);
}

}  // namespace ddpca
