// The plan of Interface::BUILD (mortar_plan.hpp): plain host C++, no HIP.  Every layout below is
// BUILD's own (mcontact.cpp), restated so that the positions can be handed to a kernel; BUILD stays
// the specification and the CPU tests compare the two byte for byte.
#include "mortar_plan.hpp"

#include <algorithm>
#include <climits>
#include <numeric>
#include <string>

#include "../../include/ddpca_amd.h"
#include "common.hpp"

namespace ddpca {

int32_t mortar_i32(int64_t v, const char* what) {
    if (v < 0 || v > INT32_MAX)
        throw ApiError(DDPCA_EINVAL, std::string("mortar plan: ") + what + " (" + std::to_string(v) + ") does not fit int32");
    return (int32_t)v;
}

namespace {

void regular_ptr(Csr& m, int64_t nrow, int64_t ncol, int64_t per) {
    m.nrow = nrow;
    m.ncol = ncol;
    m.ptr.resize(nrow + 1);
    for (int64_t r = 0; r <= nrow; ++r) m.ptr[r] = per * r;
    m.col.resize(per * nrow);
}

void build_side(const MortarInput& in, int s, MortarSide& S) {
    const int C = in.C;
    const int64_t nip = in.nip, nn = in.nn[s];
    if (nn < 0 || nip < 0) throw ApiError(DDPCA_EINVAL, "mortar plan: negative count");
    S.nn = nn;
    S.nip = nip;
    S.ninc = mortar_i32(4 * nip, "the incidence entries, 4 per point");
    mortar_i32(3 * nn, "the nodal columns, 3 per node");
    // ---- nodeCont in insertion order, ipc
    std::vector<int32_t> rowc((size_t)nn, -1);  // body node -> contact index
    S.ipc.resize(4 * nip);
    for (int64_t q = 0; q < nip; ++q)
        for (int k = 0; k < 4; ++k) {
            const int64_t n = in.ip[q].node[s][k];
            if (n < 0 || n >= nn)
                throw ApiError(DDPCA_EINVAL, "mortar plan: point " + std::to_string(q) + " names node " + std::to_string(n) +
                                                 " of side " + std::to_string(s) + ", which has " + std::to_string(nn) + " nodes");
            if (rowc[n] < 0) {
                rowc[n] = (int32_t)S.nodeCont.size();
                S.nodeCont.push_back(n);
            }
            S.ipc[4 * q + k] = rowc[n];
        }
    const int64_t ncn = S.ncn = (int64_t)S.nodeCont.size();
    const int64_t mc = C * ncn;
    // ---- the incidence list (a counting sort keeps q, then a, ascending within a node)
    S.inc_ptr.assign(ncn + 1, 0);
    for (int64_t e = 0; e < 4 * nip; ++e) ++S.inc_ptr[S.ipc[e] + 1];
    for (int64_t c = 0; c < ncn; ++c) S.inc_ptr[c + 1] += S.inc_ptr[c];
    S.inc.resize(4 * nip);
    S.inc_node.resize(4 * nip);
    {
        std::vector<int32_t> fill(S.inc_ptr.begin(), S.inc_ptr.end() - 1);
        for (int64_t e = 0; e < 4 * nip; ++e) {
            const int32_t c = S.ipc[e], w = fill[c]++;
            S.inc[w] = (int32_t)e;
            S.inc_node[w] = c;
        }
    }
    // ---- partners: sorted, unique
    std::vector<std::vector<int32_t>> part(ncn);
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t c = 0; c < ncn; ++c) {
        std::vector<int32_t>& p = part[c];
        for (int32_t e = S.inc_ptr[c]; e < S.inc_ptr[c + 1]; ++e) {
            const int64_t q = S.inc[e] >> 2;
            for (int b = 0; b < 4; ++b) p.push_back(S.ipc[4 * q + b]);
        }
        std::sort(p.begin(), p.end());
        p.erase(std::unique(p.begin(), p.end()), p.end());
    }
    int64_t npair = 0;
    for (int64_t c = 0; c < ncn; ++c) npair += (int64_t)part[c].size();
    S.npair = mortar_i32(npair, "the contact-node pairs");
    S.pptr.assign(ncn + 1, 0);
    for (int64_t c = 0; c < ncn; ++c) S.pptr[c + 1] = S.pptr[c] + (int32_t)part[c].size();
    S.part.resize(npair);
    S.pair_node.resize(npair);
    S.bypos.resize(npair);
    S.byrank.resize(npair);
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t c = 0; c < ncn; ++c) {
        const int32_t p0 = S.pptr[c], np = (int32_t)part[c].size();
        std::copy(part[c].begin(), part[c].end(), S.part.begin() + p0);
        std::fill(S.pair_node.begin() + p0, S.pair_node.begin() + p0 + np, (int32_t)c);
        // partners ordered by body node id (distinct keys: no tie to break)
        int32_t* by = S.bypos.data() + p0;
        std::iota(by, by + np, 0);
        std::sort(by, by + np, [&](int32_t x, int32_t y) { return S.nodeCont[part[c][x]] < S.nodeCont[part[c][y]]; });
        for (int32_t t = 0; t < np; ++t) S.byrank[p0 + by[t]] = t;
    }
    S.nrow0.assign(ncn, 0);
    {
        int64_t before = 0;
        for (int64_t n = 0; n < nn; ++n) {
            const int32_t a = rowc[n];
            if (a < 0) continue;
            S.nrow0[a] = (int32_t)before;
            before += S.pptr[a + 1] - S.pptr[a];
        }
    }
    // ---- the rotation table
    S.rotidx.assign(ncn, -1);
    if (in.rot[s] && !in.rot[s]->empty())
        for (int64_t c = 0; c < ncn; ++c) {
            const auto it = in.rot[s]->find(S.nodeCont[c]);
            if (it == in.rot[s]->end()) continue;
            S.rotidx[c] = (int32_t)(S.rot.size() / 9);
            S.rot.insert(S.rot.end(), it->second.begin(), it->second.end());
        }
    S.rotated = !S.rot.empty();
    // ---- nodal-space rows (3 nn): systMass (cols 3 nn), systTran(_pena) (cols mc)
    auto nodal = [&](bool mass) {
        Csr m;
        m.nrow = 3 * nn;
        m.ncol = mass ? 3 * nn : mc;
        m.ptr.assign(3 * nn + 1, 0);
        const int64_t cw = (mass || C == 3) ? 3 : 1;
        for (int64_t n = 0; n < nn; ++n) {
            const int32_t a = rowc[n];
            const int64_t per = a < 0 ? 0 : (int64_t)(S.pptr[a + 1] - S.pptr[a]) * cw;
            for (int i = 0; i < 3; ++i) m.ptr[3 * n + i + 1] = m.ptr[3 * n + i] + per;
        }
        m.col.resize(m.ptr[3 * nn]);
#pragma omp parallel for schedule(dynamic, 64)
        for (int64_t a = 0; a < ncn; ++a) {
            const int64_t n = S.nodeCont[a];
            const int32_t p0 = S.pptr[a], np = S.pptr[a + 1] - p0;
            for (int i = 0; i < 3; ++i) {
                int64_t w = m.ptr[3 * n + i];
                for (int32_t t = 0; t < np; ++t) {
                    const int32_t cb = S.part[p0 + (mass ? S.bypos[p0 + t] : t)];
                    if (mass) {
                        const int64_t nb = S.nodeCont[cb];
                        for (int j = 0; j < 3; ++j) m.col[w++] = (int32_t)(3 * nb + j);
                    } else if (C == 3) {
                        for (int j = 0; j < 3; ++j) m.col[w++] = (int32_t)(3 * cb + j);
                    } else {
                        m.col[w++] = cb;
                    }
                }
            }
        }
        return m;
    };
    S.systMass = nodal(true);
    S.systTran = nodal(false);
    S.systTran_pena = S.systTran;
    // ---- contact-space rows (mc): inteMass(_pena)
    {
        Csr& m = S.inteMass;
        m.nrow = m.ncol = mc;
        m.ptr.assign(mc + 1, 0);
        for (int64_t a = 0; a < ncn; ++a)
            for (int i = 0; i < C; ++i) m.ptr[C * a + i + 1] = m.ptr[C * a + i] + (int64_t)(S.pptr[a + 1] - S.pptr[a]) * C;
        m.col.resize(m.ptr[mc]);
#pragma omp parallel for schedule(dynamic, 64)
        for (int64_t a = 0; a < ncn; ++a)
            for (int i = 0; i < C; ++i) {
                int64_t w = m.ptr[C * a + i];
                for (int32_t k = S.pptr[a]; k < S.pptr[a + 1]; ++k)
                    for (int j = 0; j < C; ++j) m.col[w++] = (int32_t)(C * S.part[k] + j);
            }
        S.inteMass_pena = m;
    }
    // ---- per-point operators: inpoLagr (C nip x mc), inpoDisp (C nip x 3 nn), inteInpo (mc x C nip)
    regular_ptr(S.inpoLagr, C * nip, mc, 4 * C);
    regular_ptr(S.inpoDisp, C * nip, 3 * nn, 12);
    S.ord_c.resize(4 * nip);
    S.ord_n.resize(4 * nip);
#pragma omp parallel for schedule(static)
    for (int64_t q = 0; q < nip; ++q) {
        const IntegralPoint& p = in.ip[q];
        // BUILD's own two sorts, ties (a collapsed quad) included
        int ord_c[4] = {0, 1, 2, 3}, ord_n[4] = {0, 1, 2, 3};
        std::sort(ord_c, ord_c + 4, [&](int x, int y) { return S.ipc[4 * q + x] < S.ipc[4 * q + y]; });
        std::sort(ord_n, ord_n + 4, [&](int x, int y) { return p.node[s][x] < p.node[s][y]; });
        for (int t = 0; t < 4; ++t) S.ord_c[4 * q + t] = (uint8_t)ord_c[t], S.ord_n[4 * q + t] = (uint8_t)ord_n[t];
        for (int m = 0; m < C; ++m) {
            const int64_t r = C * q + m;
            int64_t wl = S.inpoLagr.ptr[r], wd = S.inpoDisp.ptr[r];
            for (int t = 0; t < 4; ++t) {
                const int a = ord_c[t];
                if (C == 1) {
                    S.inpoLagr.col[wl++] = S.ipc[4 * q + a];
                } else {
                    for (int k = 0; k < 3; ++k) S.inpoLagr.col[wl++] = 3 * S.ipc[4 * q + a] + k;
                }
                const int an = ord_n[t];
                for (int k = 0; k < 3; ++k) S.inpoDisp.col[wd++] = (int32_t)(3 * p.node[s][an] + k);
            }
        }
    }
    S.pemaInpo_r = S.inpoDisp;
    {
        Csr& m = S.inteInpo;
        m.nrow = mc;
        m.ncol = C * nip;
        m.ptr.assign(mc + 1, 0);
        for (int64_t c = 0; c < ncn; ++c)
            for (int k = 0; k < C; ++k) m.ptr[C * c + k + 1] = m.ptr[C * c + k] + (int64_t)C * (S.inc_ptr[c + 1] - S.inc_ptr[c]);
        m.col.resize(m.ptr[mc]);
#pragma omp parallel for schedule(static)
        for (int64_t e = 0; e < 4 * nip; ++e) {
            const int32_t c = S.inc_node[e];
            const int64_t q = S.inc[e] >> 2, r = e - S.inc_ptr[c];
            for (int k = 0; k < C; ++k)
                for (int mm = 0; mm < C; ++mm) m.col[m.ptr[C * c + k] + C * r + mm] = (int32_t)(C * q + mm);
        }
    }
}

}  // namespace

mortar::MortarView MortarSide::view(int s, int C, double penN, double penF) const {
    mortar::MortarView V;
    V.s = s;
    V.nip = nip, V.ncn = ncn, V.npair = npair, V.ninc = ninc;
    V.pen[0] = penN, V.pen[1] = penF, V.pen[2] = penF;
    V.ipc = ipc.data(), V.inc_ptr = inc_ptr.data(), V.inc = inc.data(), V.inc_node = inc_node.data();
    V.pptr = pptr.data(), V.part = part.data(), V.pair_node = pair_node.data(), V.byrank = byrank.data();
    V.nrow0 = nrow0.data(), V.rotidx = rotidx.data(), V.ord_c = ord_c.data(), V.ord_n = ord_n.data();
    V.rot = rot.data();
    V.n_mass = systMass.nnz(), V.n_tran = systTran.nnz(), V.n_imass = inteMass.nnz();
    V.n_lagr = inpoLagr.nnz(), V.n_disp = inpoDisp.nnz(), V.n_inpo = inteInpo.nnz();
    (void)C;
    return V;
}

MortarPlan mortar_plan(const MortarInput& in) {
    if (in.C != 1 && in.C != 3) throw ApiError(DDPCA_EINVAL, "mortar plan: comp() is 1 or 3");
    if (in.nip > 0 && !in.ip) throw ApiError(DDPCA_EINVAL, "mortar plan: null points");
    static_assert(sizeof(IntegralPoint) == 8 * mortar::kPointWords, "IntegralPoint is 27 words of 8 bytes");
    MortarPlan P;
    P.C = in.C;
    for (int s = 0; s < 2; ++s) build_side(in, s, P.side[s]);
    P.factored = !P.side[0].rotated && !P.side[1].rotated;
    return P;
}

void mortar_finish(const MortarInput& in, MortarPlan& P, MortarValues (&val)[2], Interface& itf) {
    const int C = in.C;
    for (int s = 0; s < 2; ++s) {
        MortarSide& S = P.side[s];
        MortarValues& v = val[s];
        auto take = [](Csr& dst, Csr& pat, std::vector<double>& values) {
            dst = std::move(pat);
            dst.val = std::move(values);
        };
        itf.nodeCont[s] = std::move(S.nodeCont);
        take(itf.systMass[s], S.systMass, v.mass);
        take(itf.systTran[s], S.systTran, v.tran);
        take(itf.systTran_pena[s], S.systTran_pena, v.tranp);
        take(itf.inteMass[s], S.inteMass, v.imass);
        take(itf.inteMass_pena[s], S.inteMass_pena, v.imassp);
        take(itf.inpoLagr[s], S.inpoLagr, v.lagr);
        take(itf.inpoDisp[s], S.inpoDisp, v.disp);
        take(itf.inteInpo[s], S.inteInpo, v.inpo);
        take(itf.pemaInpo_r[s], S.pemaInpo_r, v.pema);
    }
    itf.factored = P.factored;
    const double pen[3] = {in.penN, in.penF, in.penF};
    itf.inpoNgap.assign(C * in.nip, 0.0);
    itf.pemaDiag.assign(C * in.nip, 0.0);
    for (int64_t q = 0; q < in.nip; ++q) {
        itf.inpoNgap[C * q] = in.ip[q].gap;
        for (int m = 0; m < C; ++m) itf.pemaDiag[C * q + m] = pen[m];
    }
}

MortarInput mortar_input(const Interface& itf, const int64_t nn[2], const NodeRota* const rot[2]) {
    MortarInput in;
    in.ip = itf.ip.data();
    in.nip = (int64_t)itf.ip.size();
    in.C = itf.comp();
    in.penN = itf.penN;
    in.penF = itf.penF;
    for (int s = 0; s < 2; ++s) in.nn[s] = nn[s], in.rot[s] = rot ? rot[s] : nullptr;
    return in;
}

}  // namespace ddpca
