// C ABI of the mortar operators with a chosen path (Interface::BUILD: MCONTACT.h:181-810, CONT_ROTA
// 157-179): ddpca_interface_build_on on points of the caller (device >= 0: the kernels of
// device_mortar.hip; -1: Interface::BUILD, unchanged; -2: the device path's own steps on the host),
// ddpca_problem_set_mortar_device, which hands the interfaces of MCONTACT::ESTABLISH to the device,
// ddpca_problem_set_ips_from and the measurement getter.
#include <chrono>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/ddpca_amd.h"
#include "device_common.hpp"
#include "device_csearch.hpp"  // ddpca_ips
#include "device_mortar.hpp"
#include "problem.hpp"

using namespace ddpca;

struct ddpca_interface {
    Interface itf;
    std::vector<int64_t> shape, factored;
};

namespace {

// of the calling thread's last device build (device >= 0): plan, uploads and allocations,
// k_mortar_pair, k_mortar_nodal + k_mortar_ip, copy back
thread_local double last_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};

void build_by(int device, Interface& itf, const int64_t nn[2], const NodeRota* const rot[2]) {
    const MortarInput in = mortar_input(itf, nn, rot);
    if (device == -2) {
        mortar_build_host(in, itf);
        return;
    }
    select_device(device);
    mortar_build_device(in, itf, last_ms);
}

template <typename T>
void put(const std::vector<T>& v, int code, const void** data, int64_t* count, int* dtype) {
    *data = v.data();
    *count = (int64_t)v.size();
    *dtype = code;
}

NodeRota rota_of(int64_t nrot, const int64_t* node, const double* rot, int64_t nn, const char* who) {
    if (nrot < 0 || (nrot > 0 && (!node || !rot))) throw ApiError(DDPCA_EINVAL, std::string(who) + ": null rotation arrays");
    NodeRota m;
    for (int64_t k = 0; k < nrot; ++k) {
        if (node[k] < 0 || node[k] >= nn) throw ApiError(DDPCA_EINVAL, std::string(who) + ": rotated node id out of range");
        std::array<double, 9> R;
        std::memcpy(R.data(), rot + 9 * k, sizeof(double) * 9);
        m[node[k]] = R;
    }
    return m;
}

}  // namespace

extern "C" {

// MCONTACT.h:181-810, 157-179
int ddpca_interface_build_on(int device, int64_t nn0, int64_t nn1, double fric, double penN, double penF, int64_t nip,
                             const int64_t* node, const double* shap, const double* basis, const double* gap, const double* w,
                             int64_t nrot0, const int64_t* rot_node0, const double* rot0, int64_t nrot1,
                             const int64_t* rot_node1, const double* rot1, ddpca_interface_t* out) {
    return guarded([&] {
        const char* who = "ddpca_interface_build_on";
        if (!out || nip < 0 || nn0 < 0 || nn1 < 0 || (nip > 0 && (!node || !shap || !basis || !gap || !w)))
            throw ApiError(DDPCA_EINVAL, std::string(who) + ": null argument or negative count");
        if (device < -2) throw ApiError(DDPCA_EINVAL, std::string(who) + ": device is an index >= 0, -1 (host) or -2 (device path on the host)");
        const int64_t nn[2] = {nn0, nn1};
        auto h = std::make_unique<ddpca_interface>();
        Interface& itf = h->itf;
        itf.fric = fric;
        itf.penN = penN;
        itf.penF = penF;
        itf.ip.resize(nip);
        for (int64_t q = 0; q < nip; ++q) {
            IntegralPoint& p = itf.ip[q];
            for (int s = 0; s < 2; ++s)
                for (int k = 0; k < 4; ++k) {
                    p.node[s][k] = node[8 * q + 4 * s + k];
                    p.shap[s][k] = shap[8 * q + 4 * s + k];
                    if (p.node[s][k] < 0 || p.node[s][k] >= nn[s])
                        throw ApiError(DDPCA_EINVAL, std::string(who) + ": point " + std::to_string(q) + " names node " +
                                                         std::to_string(p.node[s][k]) + " of side " + std::to_string(s) +
                                                         ", which has " + std::to_string(nn[s]) + " nodes");
                }
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) p.basis[a][b] = basis[9 * q + 3 * a + b];
            p.gap = gap[q];
            p.w = w[q];
        }
        const NodeRota r0 = rota_of(nrot0, rot_node0, rot0, nn0, who), r1 = rota_of(nrot1, rot_node1, rot1, nn1, who);
        const NodeRota* const rot[2] = {&r0, &r1};
        if (device == -1) itf.BUILD(nn, rot);
        else build_by(device, itf, nn, rot);
        *out = h.release();
    });
}

// MCONTACT.h:181-810, 157-179
int ddpca_interface_view(ddpca_interface_t h, const char* cname, int side, const void** data, int64_t* count, int* dtype) {
    return guarded([&] {
        if (!h || !cname || !data || !count || !dtype) throw ApiError(DDPCA_EINVAL, "ddpca_interface_view: null argument");
        const std::string name(cname);
        Interface& itf = h->itf;
        if (name == "factored") {
            h->factored = {itf.factored ? 1 : 0};
            put(h->factored, 1, data, count, dtype);
            return;
        }
        if (name == "inpoNgap") { put(itf.inpoNgap, 0, data, count, dtype); return; }
        if (name == "pemaDiag") { put(itf.pemaDiag, 0, data, count, dtype); return; }
        if (side < 0 || side > 1) throw ApiError(DDPCA_EINVAL, "ddpca_interface_view: side is 0 or 1");
        const int s = side;
        if (name == "nodeCont") { put(itf.nodeCont[s], 1, data, count, dtype); return; }
        const size_t colon = name.find(':');
        const std::string b = name.substr(0, colon), part = colon == std::string::npos ? "" : name.substr(colon + 1);
        const Csr* m = nullptr;
        if (b == "systMass") m = &itf.systMass[s];
        if (b == "systTran") m = &itf.systTran[s];
        if (b == "systTran_pena") m = &itf.systTran_pena[s];
        if (b == "inteMass") m = &itf.inteMass[s];
        if (b == "inteMass_pena") m = &itf.inteMass_pena[s];
        if (b == "inpoLagr") m = &itf.inpoLagr[s];
        if (b == "inpoDisp") m = &itf.inpoDisp[s];
        if (b == "inteInpo") m = &itf.inteInpo[s];
        if (b == "pemaInpo_r") m = &itf.pemaInpo_r[s];
        if (!m) throw ApiError(DDPCA_EINVAL, "ddpca_interface_view: unknown array " + name);
        if (part == "ptr") put(m->ptr, 1, data, count, dtype);
        else if (part == "col") put(m->col, 2, data, count, dtype);
        else if (part == "val") put(m->val, 0, data, count, dtype);
        else if (part == "shape") {
            h->shape = {m->nrow, m->ncol};
            put(h->shape, 1, data, count, dtype);
        } else {
            throw ApiError(DDPCA_EINVAL, "ddpca_interface_view: unknown array " + name);
        }
    });
}

// MCONTACT.h:181-810, 157-179
int ddpca_interface_destroy(ddpca_interface_t h) {
    return guarded([&] { delete h; });
}

// MCONTACT.h:181-810, 157-179 (from MCONTACT::ESTABLISH, 812-825)
int ddpca_problem_set_mortar_device(ddpca_problem_t p, int device) {
    return guarded([&] {
        if (!p) throw ApiError(DDPCA_EINVAL, "ddpca_problem_set_mortar_device: null problem");
        Problem& P = *reinterpret_cast<Problem*>(p);
        if (P.established) throw ApiError(DDPCA_ESTATE, "ddpca_problem_set_mortar_device: problem already established");
        if (device < 0) {
            P.mc.mortarBy = nullptr;
            return;
        }
        select_device(device);
        P.mc.mortarBy = [device](Interface& itf, const int64_t nn[2], const NodeRota* const rot[2]) {
            build_by(device, itf, nn, rot);
        };
    });
}

// MCONTACT.h:181-810, 157-179 (measurement only)
int ddpca_mortar_last_ms(double* out5) {
    return guarded([&] {
        if (!out5) throw ApiError(DDPCA_EINVAL, "ddpca_mortar_last_ms: null argument");
        for (int k = 0; k < 5; ++k) out5[k] = last_ms[k];
    });
}

// MCONTACT.h:181-810 (the points BUILD reads; CSEARCH.h:19-32)
int ddpca_problem_set_ips_from(ddpca_problem_t p, int64_t ts, ddpca_ips_t h, double fric, double penN, double penF) {
    return guarded([&] {
        if (!p || !h) throw ApiError(DDPCA_EINVAL, "ddpca_problem_set_ips_from: null argument");
        Problem& P = *reinterpret_cast<Problem*>(p);
        if (ts < 0 || ts >= (int64_t)P.mc.searCont.size()) throw ApiError(DDPCA_EINVAL, "interface index");
        if (P.established) throw ApiError(DDPCA_ESTATE, "set_ips after establish");
        if (h->n > 0 && !h->values) throw ApiError(DDPCA_ESTATE, "ddpca_problem_set_ips_from: this search kept the node ids only");
        Interface& itf = P.mc.searCont[ts];
        const int64_t n = h->n;
        itf.ip.resize(n);
#pragma omp parallel for schedule(static)
        for (int64_t q = 0; q < n; ++q) {
            IntegralPoint& ip = itf.ip[q];
            std::memcpy(ip.node, h->node.get() + 8 * q, sizeof ip.node);
            std::memcpy(ip.shap, h->shap.get() + 8 * q, sizeof ip.shap);
            std::memcpy(ip.basis, h->basis.get() + 9 * q, sizeof ip.basis);
            ip.gap = h->gap[q];
            ip.w = h->w[q];
        }
        itf.fric = fric;
        itf.penN = penN;
        itf.penF = penF;
    });
}

}  // extern "C"
