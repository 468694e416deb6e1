// Host setup of the ADMM handle: see admm_plan.hpp.
#include "admm_plan.hpp"

#include <array>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <string>
#include <unordered_map>

#include "common.hpp"
#include "csr_ops.hpp"
#include "mgpis_layout.hpp"  // pad64

namespace ddpca {

AdmmTuning admm_tuning() {
    AdmmTuning t;
    if (const char* e = std::getenv("DDPCA_MASS_FUSED")) t.mass_fused = std::atoi(e) != 0;
    if (const char* e = std::getenv("DDPCA_COARSE_MG_MIN")) t.coarse_mg_min = std::atoll(e);
    if (const char* e = std::getenv("DDPCA_COARSE_DENSE_MB")) t.coarse_dense_mb = std::atof(e);
    if (const char* e = std::getenv("DDPCA_PCG_MAXIT")) t.pcg_maxit = std::atoll(e);
    t.verbose = std::getenv("DDPCA_VERBOSE") != nullptr;
    return t;
}

int32_t w32(int64_t w) {
    if (w < 0 || w > INT32_MAX) throw ApiError(DDPCA_EINVAL, "workspace index exceeds int32");
    return (int32_t)w;
}

void sum_duplicates(std::vector<std::pair<int32_t, double>>& row) {
    std::stable_sort(row.begin(), row.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    size_t out = 0;
    for (size_t e = 0; e < row.size();) {
        size_t f = e;
        double v = 0.0;
        for (; f < row.size() && row[f].first == row[e].first; ++f) v += row[f].second;
        row[out++] = {row[e].first, v};
        e = f;
    }
    row.resize(out);
}

Csr triplets_to_csr(const std::vector<double>& trip, int64_t ntrip, int64_t n) {
    std::vector<std::vector<std::pair<int32_t, double>>> rows(n);
    for (int64_t q = 0; q < ntrip; ++q) {
        const int64_t r = (int64_t)trip[3 * q], c = (int64_t)trip[3 * q + 1];
        if (r < 0 || r >= n || c < 0 || c >= n) throw ApiError(DDPCA_EINVAL, "gathered coarse operator: an entry outside the matrix");
        rows[r].push_back({(int32_t)c, trip[3 * q + 2]});
    }
    Csr A;
    A.nrow = A.ncol = n;
    A.ptr.assign(1, 0);
    for (auto& row : rows) {
        sum_duplicates(row);
        for (const auto& e : row) {
            A.col.push_back(e.first);
            A.val.push_back(e.second);
        }
        A.ptr.push_back((int64_t)A.col.size());
    }
    return A;
}

SellPlan sell_pack(const Rows& rows) {
    SellPlan P;
    const int64_t nr = (int64_t)rows.size();
    P.nrow = pad64(nr);
    P.nch = P.nrow / 64;
    P.slots.assign(std::max<int64_t>(P.nch, 1), 0);
    P.off.assign(P.nch + 1, 0);
    for (int64_t c = 0; c < P.nch; ++c) {
        size_t mx = 0;
        for (int64_t r = c * 64; r < std::min<int64_t>(nr, (c + 1) * 64); ++r) mx = std::max(mx, rows[r].size());
        P.slots[c] = (int32_t)mx;
        P.off[c + 1] = P.off[c] + (int64_t)mx;
    }
    P.col.assign(std::max<int64_t>(P.off[P.nch] * 64, 1), 0);
    P.val.assign(std::max<int64_t>(P.off[P.nch] * 64, 1), 0.0);
    int64_t ent = 0;
    std::vector<int64_t> cols;
    for (int64_t r = 0; r < nr; ++r) {
        const int64_t c = r / 64, lane = r % 64;
        ent += (int64_t)rows[r].size();
        for (size_t k = 0; k < rows[r].size(); ++k) {
            P.col[(P.off[c] + (int64_t)k) * 64 + lane] = w32(rows[r][k].first);
            P.val[(P.off[c] + (int64_t)k) * 64 + lane] = rows[r][k].second;
            cols.push_back(rows[r][k].first);
        }
    }
    P.bytes = 12.0 * (double)ent + 8.0 * (double)count_distinct(std::move(cols)) + 8.0 * (double)nr;
    return P;
}

// ------------------------------------------------------------------------------- tables
std::vector<AdmmSub> owned_subdomains(const Problem& P, const std::vector<int32_t>& owner, int rank) {
    const int64_t nsub = (int64_t)P.mc.multGrid.size();
    std::vector<AdmmSub> subs;
    for (int64_t tv = 0; tv < nsub; ++tv) {
        if (owner[tv] != rank) continue;
        if (P.owned.size() != (size_t)nsub || !P.owned[tv])
            throw ApiError(DDPCA_ESTATE, "subdomain " + std::to_string(tv) + " is owned by this rank but was not established");
        const MULTIGRID& g = P.mc.multGrid[tv];
        AdmmSub S;
        S.tv = tv;
        S.nn = g.leveCount.back();
        S.nh = 3 * (g.nodalCount() - S.nn);
        subs.push_back(S);
    }
    return subs;
}

AdmmTables plan_tables(const MCONTACT& mc, std::vector<AdmmSub> subs, const std::vector<int32_t>& owner, int rank,
                       const BatchView& V, const AdmmTuning& tune) {
    AdmmTables T;
    T.nsub = (int64_t)mc.multGrid.size();
    T.nint = (int64_t)mc.searCont.size();
    T.subs = std::move(subs);
    if (V.empty() != T.subs.empty()) throw ApiError(DDPCA_ESTATE, "the batch does not hold the owned subdomains");
    const int64_t NN = V.empty() ? 0 : V.lev.back().nn;
    T.NU = std::max<int64_t>(3 * NN, 64);
    for (auto& S : T.subs) {
        S.hoff = T.NH;
        T.NH += S.nh;
    }
    T.NH = pad64(T.NH);
    T.cf.assign(T.NU, 0.0);
    T.presc.assign(T.NU, 0.0);
    T.onode.resize(std::max<int64_t>(NN, 1));
    std::iota(T.onode.begin(), T.onode.end(), 0);  // padding nodes map to themselves
    for (size_t i = 0; i < T.subs.size(); ++i) {
        auto& S = T.subs[i];
        S.dof0 = V.fine_dof_offset((int)i);
        T.maxit.push_back(tune.pcg_maxit > 0 ? std::min<int64_t>(tune.pcg_maxit, V.nfree[i]) : V.nfree[i]);
        const MULTIGRID& g = mc.multGrid[S.tv];
        for (int64_t d = 0; d < 3 * S.nn; ++d)
            if (g.consFlag[d]) T.cf[V.fine_dof((int)i, d)] = g.consForc[g.freeIndex[d]];
        for (const auto& kv : g.consDofv) T.presc[S.dof0 + kv.first] = kv.second;
        const auto& perm = V.fine_perm((int)i);
        for (int64_t r = 0; r < S.nn; ++r) T.onode[S.dof0 / 3 + perm[r]] = w32(S.dof0 / 3 + r);
    }
    auto sub_index = [&](int64_t tv) {
        for (size_t i = 0; i < T.subs.size(); ++i)
            if (T.subs[i].tv == tv) return (int)i;
        return -1;
    };
    // ---- owned interface sides: aux rows [roff, roff + m), lambda rows R + the same
    int64_t roff = 0;
    for (int64_t ts = 0; ts < T.nint; ++ts) {
        const Interface& itf = mc.searCont[ts];
        for (int s = 0; s < 2; ++s) {
            if (owner[itf.body[s]] != rank) continue;
            AdmmSide sd;
            sd.ts = ts;
            sd.s = s;
            sd.tv = itf.body[s];
            sd.sub = sub_index(sd.tv);
            sd.m = itf.mside(s);
            sd.mip = itf.mip();
            sd.roff = roff;
            roff += pad64(sd.m);
            T.side_of[{ts, s}] = T.sides.size();
            T.sides.push_back(sd);
        }
    }
    T.R = roff;
    // ---- interfaces: gamma layout (cross-rank interfaces first, then rank-local)
    int64_t goff = 0;
    T.itfs.resize(T.nint);
    for (int pass = 0; pass < 2; ++pass)
        for (int64_t ts = 0; ts < T.nint; ++ts) {
            const Interface& itf = mc.searCont[ts];
            const int o0 = owner[itf.body[0]], o1 = owner[itf.body[1]];
            const bool cross = o0 != o1;
            if ((pass == 0) != cross) continue;
            AdmmItf& I = T.itfs[ts];
            I.ts = ts;
            I.mip = itf.mip();
            I.comp = itf.comp();
            I.fric = itf.fric;
            I.owner[0] = o0;
            I.owner[1] = o1;
            I.cross = cross;
            I.mine = (o0 == rank || o1 == rank);
            I.goff = goff;
            goff += I.mip;
        }
    T.G = pad64(std::max<int64_t>(goff, 1));
    T.oH = T.NU;
    T.oS = T.NU + T.NH;
    T.oG = T.oS + 2 * T.R;
    w32(T.oG + T.G - 1);  // every workspace index fits the kernels' int32 columns
    return T;
}

// ------------------------------------------------------------------------------- factored per-ip operands
FactItfPlan plan_factored(const MCONTACT& mc, const AdmmTables& T, const AdmmItf& I) {
    const Interface& itf = mc.searCont[I.ts];
    FactItfPlan F;
    F.ts = I.ts;
    F.nip = (int64_t)itf.ip.size();
    F.goff = I.goff;
    F.C = itf.comp();
    for (int m = 0; m < F.C; ++m) F.pen[m] = itf.pemaDiag[m];  // pemaDiag[C q + m] = pen[m] for every q
    const int64_t nip = F.nip, np = std::max<int64_t>(nip, 1);
    F.B.resize(9 * np);
    for (int64_t q = 0; q < nip; ++q)
        for (int j = 0; j < 9; ++j) F.B[j * nip + q] = itf.ip[q].basis[j / 3][j % 3];
    for (int s = 0; s < 2; ++s) {
        const auto own = T.side_of.find({I.ts, s});
        if (own == T.side_of.end()) continue;
        F.own[s] = 1;
        const auto& sd = T.sides[own->second];
        const auto& Su = T.subs[sd.sub];
        const int64_t lam0 = T.oS + T.R + sd.roff;
        std::unordered_map<int64_t, int32_t> cidx;
        for (size_t a = 0; a < itf.nodeCont[s].size(); ++a) cidx.emplace(itf.nodeCont[s][a], (int32_t)a);
        F.M[s].resize(4 * np);
        F.lam[s].resize(4 * np);
        F.u[s].resize(4 * np);
        std::vector<std::vector<std::pair<int32_t, double>>> bynode(itf.nodeCont[s].size());
        const double sgn = s == 0 ? -1.0 : 1.0;  // inteInpo's sign (mcontact.cpp BUILD)
        for (int64_t q = 0; q < nip; ++q)
            for (int a = 0; a < 4; ++a) {
                const int64_t node = itf.ip[q].node[s][a];
                const int32_t c = cidx.at(node);
                F.M[s][a * nip + q] = itf.ip[q].shap[s][a];
                F.lam[s][a * nip + q] = w32(lam0 + F.C * c);
                F.u[s][a * nip + q] = w32(Su.wcol(3 * node, T.oH));
                bynode[c].push_back({(int32_t)q, sgn * (itf.ip[q].w * itf.ip[q].shap[s][a])});
            }
        F.nptr[s].assign(1, 0);
        for (const auto& v : bynode) {
            for (const auto& e : v) {
                F.niq[s].push_back(e.first);
                F.ncoef[s].push_back(e.second);
            }
            F.nptr[s].push_back((int64_t)F.niq[s].size());
        }
        F.nnc[s] = (int64_t)bynode.size();
        F.roff[s] = sd.roff;
        // k_gamma_ip's share of this side: shape values, lambda and u indices per ip, the
        // side's contact-node lambda (C per node) and body-node u (3 per node) once;
        // k_inpo_node: index + coefficient per (node, ip) entry, the node's C outputs
        F.bytes_gamma += 48.0 * (double)nip + (double)F.nnc[s] * 8.0 * (F.C + 3);
        F.bytes_inpo += 12.0 * (double)F.niq[s].size() + 8.0 * F.C * (double)nip + 8.0 * F.C * (double)F.nnc[s];
        if (F.niq[s].empty()) {  // (never an empty device buffer)
            F.niq[s].assign(1, 0);
            F.ncoef[s].assign(1, 0.0);
        }
    }
    // per ip: the 3x3 basis, gamma written and the constant part read (k_gamma_ip); basis,
    // gamma read and the traction written (k_traction_ip)
    F.bytes_gamma += (double)nip * (72.0 + 16.0 * F.C);
    F.bytes_inpo += (double)nip * ((F.C == 3 ? 72.0 : 0.0) + 16.0 * F.C);
    return F;
}

// ------------------------------------------------------------------------------- interface operators
bool fused_update(const MCONTACT& mc, const AdmmTables& T, const AdmmTuning& tune) {
    // (entries agree to rounding: the penalty operators are accumulated with pen inside the
    // basis products, e.g. off-diagonal T^T P T entries are rounding noise around 0)
    auto proportional = [](const Csr& A, const Csr& B, double rho) {
        if (A.nrow != B.nrow || A.ptr != B.ptr || A.col != B.col) return false;
        double amax = 0.0;
        for (double v : A.val) amax = std::max(amax, std::abs(v));
        for (int64_t k = 0; k < A.nnz(); ++k)
            if (std::abs(A.val[k] - rho * B.val[k]) > 1e-13 * amax) return false;
        return true;
    };
    bool fuse = !T.sides.empty() && tune.mass_fused;
    for (const auto& sd : T.sides) {
        const Interface& itf = mc.searCont[sd.ts];
        const double rho = itf.penN;
        fuse = fuse && itf.penN == itf.penF && rho > 0.0 && proportional(itf.inteMass_pena[sd.s], itf.inteMass[sd.s], rho) &&
               proportional(itf.systTran_pena[sd.s], itf.systTran[sd.s], rho);
    }
    return fuse;
}

AdmmOperators plan_operators(const MCONTACT& mc, const AdmmTables& T, bool fuse) {
    AdmmOperators O;
    Rows rg(T.G), ra(fuse ? 0 : T.R), rl(fuse ? 0 : T.R), rg1;
    std::map<int64_t, int64_t> g1off;  // rank-local SELL interface -> its first row in rg1
    O.gcst.assign(T.G, 0.0);
    for (const auto& sd : T.sides) {
        const Interface& itf = mc.searCont[sd.ts];
        const auto& I = T.itf_of(sd.ts);
        const int s = (int)sd.s;
        const double half = s == 0 ? 0.5 : -0.5;
        const auto& Su = T.subs[sd.sub];
        const int64_t lam0 = T.oS + T.R + sd.roff, aux0 = T.oS + sd.roff;
        // gamma half: +-1/2 (inpoLagr lambda + pemaInpo_r u); side 0 adds -1/2 pema g
        const Csr& Lg = itf.inpoLagr[s];
        const Csr& Rg = itf.pemaInpo_r[s];
        // a rank-local interface's side 1 sums its half in rows of its own (op_gamma1)
        const bool own_rows1 = !itf.factored && s == 1 && !I.cross;
        if (own_rows1 && !g1off.count(sd.ts)) {
            g1off[sd.ts] = (int64_t)rg1.size();
            for (int64_t i = 0; i < sd.mip; ++i) O.gam1_dst.push_back(w32(I.goff + i));
            rg1.resize(rg1.size() + sd.mip);
        }
        for (int64_t i = 0; i < sd.mip; ++i) {
            if (!itf.factored) {  // factored interfaces: k_gamma_ip
                auto& row = own_rows1 ? rg1[g1off[sd.ts] + i] : rg[I.goff + i];
                for (int64_t k = Lg.ptr[i]; k < Lg.ptr[i + 1]; ++k) row.push_back({lam0 + Lg.col[k], half * Lg.val[k]});
                for (int64_t k = Rg.ptr[i]; k < Rg.ptr[i + 1]; ++k) row.push_back({Su.wcol(Rg.col[k], T.oH), half * Rg.val[k]});
            }
            if (s == 0) O.gcst[I.goff + i] = -0.5 * (itf.pemaDiag[i] * itf.inpoNgap[i]);
        }
        if (fuse) continue;
        // aux RHS: systTran_pena^T u + inteMass lambda + inteInpo gamma
        const Csr tTp = csr::transpose(itf.systTran_pena[s]);
        const Csr& M = itf.inteMass[s];
        const Csr& Mp = itf.inteMass_pena[s];
        const Csr& Ii = itf.inteInpo[s];
        for (int64_t r = 0; r < sd.m; ++r) {
            auto& a = ra[sd.roff + r];
            auto& l = rl[sd.roff + r];
            for (int64_t k = tTp.ptr[r]; k < tTp.ptr[r + 1]; ++k) {
                a.push_back({Su.wcol(tTp.col[k], T.oH), tTp.val[k]});
                l.push_back({Su.wcol(tTp.col[k], T.oH), tTp.val[k]});
            }
            for (int64_t k = M.ptr[r]; k < M.ptr[r + 1]; ++k) a.push_back({lam0 + M.col[k], M.val[k]});
            for (int64_t k = Ii.ptr[r]; k < Ii.ptr[r + 1]; ++k) a.push_back({T.oG + I.goff + Ii.col[k], Ii.val[k]});
            // lambda RHS: systTran_pena^T u - inteMass_pena aux
            for (int64_t k = Mp.ptr[r]; k < Mp.ptr[r + 1]; ++k) l.push_back({aux0 + Mp.col[k], -Mp.val[k]});
        }
    }
    // each row list is dropped as soon as it is packed
    O.gamma = sell_pack(rg);
    Rows().swap(rg);
    O.has_gamma1 = !rg1.empty();
    if (O.has_gamma1) O.gamma1 = sell_pack(rg1);
    Rows().swap(rg1);
    if (!fuse) {
        O.aux = sell_pack(ra);
        Rows().swap(ra);
        O.lam = sell_pack(rl);
    }
    return O;
}

AdmmFused plan_fused(const MCONTACT& mc, const AdmmTables& T) {
    AdmmFused F;
    Rows rwv(2 * T.R);
    F.rinv.assign(std::max<int64_t>(T.R, 1), 0.0);
    for (const auto& sd : T.sides) {
        const Interface& itf = mc.searCont[sd.ts];
        const auto& I = T.itf_of(sd.ts);
        const auto& Su = T.subs[sd.sub];
        const Csr tT = csr::transpose(itf.systTran[sd.s]);
        const Csr& Ii = itf.inteInpo[sd.s];
        for (int64_t r = 0; r < sd.m; ++r) {
            for (int64_t k = tT.ptr[r]; k < tT.ptr[r + 1]; ++k) rwv[sd.roff + r].push_back({Su.wcol(tT.col[k], T.oH), tT.val[k]});
            if (!itf.factored)  // factored interfaces: k_traction_ip + k_inpo_node
                for (int64_t k = Ii.ptr[r]; k < Ii.ptr[r + 1]; ++k)
                    rwv[T.R + sd.roff + r].push_back({T.oG + I.goff + Ii.col[k], Ii.val[k]});
            F.rinv[sd.roff + r] = 1.0 / itf.penN;
        }
    }
    F.wv = sell_pack(rwv);
    return F;
}

MassList mass_list(const MCONTACT& mc, const AdmmTables& T, int which) {
    MassList L;
    for (int rep = 0; rep < (which == 2 ? 2 : 1); ++rep)
        for (const auto& sd : T.sides) {
            const Interface& itf = mc.searCont[sd.ts];
            L.A.push_back(which == 0 ? &itf.inteMass_pena[sd.s] : &itf.inteMass[sd.s]);
            L.roff.push_back(rep * T.R + sd.roff);
        }
    L.nrow = (which == 2 ? 2 : 1) * T.R;
    return L;
}

// ------------------------------------------------------------------------------- body-balance RHS
CouplingPlan plan_coupling(const MCONTACT& mc, const AdmmTables& T, const BatchView& V) {
    std::map<int64_t, std::vector<std::pair<int32_t, double>>> rowmap;
    for (size_t si = 0; si < T.subs.size(); ++si) {
        const auto& S = T.subs[si];
        const MULTIGRID& g = mc.multGrid[S.tv];
        for (int64_t ts = 0; ts < T.nint; ++ts) {
            const Interface& itf = mc.searCont[ts];
            for (int s = 0; s < 2; ++s) {
                if (itf.body[s] != S.tv) continue;
                const auto& sd = T.sides[T.side_of.at({ts, s})];
                const Csr& Tp = itf.systTran_pena[s];
                const Csr& Tr = itf.systTran[s];
                const int64_t n3 = 3 * S.nn;
                for (int64_t r = 0; r < Tp.nrow; ++r) {
                    // only the rows the interface actually couples (surface rows)
                    if (Tp.ptr[r] == Tp.ptr[r + 1] && Tr.ptr[r] == Tr.ptr[r + 1]) continue;
                    // a hanging-level row reaches the free dofs through prolOper[maxiLeve]^T
                    // (ADDITIONAL_FORCE, MULTIGRID.h:1257-1261)
                    std::vector<std::pair<int64_t, double>> tgt;
                    if (r < n3) {
                        tgt.push_back({r, 1.0});
                    } else {
                        const Csr& Hp = g.hangProl;
                        for (int64_t k = Hp.ptr[r - n3]; k < Hp.ptr[r - n3 + 1]; ++k) tgt.push_back({Hp.col[k], Hp.val[k]});
                    }
                    for (const auto& [d, w] : tgt) {
                        if (!g.consFlag[d] || w == 0.0) continue;
                        auto& row = rowmap[V.fine_dof((int)si, d)];  // added into the solver RHS
                        for (int64_t k = Tp.ptr[r]; k < Tp.ptr[r + 1]; ++k)
                            row.push_back({w32(T.oS + sd.roff + Tp.col[k]), w * Tp.val[k]});
                        for (int64_t k = Tr.ptr[r]; k < Tr.ptr[r + 1]; ++k)
                            row.push_back({w32(T.oS + T.R + sd.roff + Tr.col[k]), -w * Tr.val[k]});
                    }
                }
            }
        }
    }
    CouplingPlan P;
    P.cptr.assign(1, 0);
    for (auto& kv : rowmap) {
        P.crow.push_back(w32(kv.first));
        sum_duplicates(kv.second);  // hanging rows folded onto the same free dof
        for (const auto& e : kv.second) {
            P.ccol.push_back(e.first);
            P.cval.push_back(e.second);
        }
        P.cptr.push_back((int64_t)P.ccol.size());
    }
    // k_cpl: entries, the row's target index and pointer, b read + written, W's aux and lambda
    // entries once
    P.bytes = 12.0 * (double)P.ccol.size() + 28.0 * (double)P.crow.size() + 8.0 * (double)count_distinct(P.ccol);
    return P;
}

SellPlan plan_hanging(const MCONTACT& mc, const AdmmTables& T) {
    Rows rh(T.NH);
    for (const auto& S : T.subs) {
        const Csr& Hp = mc.multGrid[S.tv].hangProl;
        for (int64_t r = 0; r < S.nh; ++r)
            for (int64_t k = Hp.ptr[r]; k < Hp.ptr[r + 1]; ++k) rh[S.hoff + r].push_back({S.wcol(Hp.col[k], T.oH), Hp.val[k]});
    }
    return sell_pack(rh);
}

AdmmBytes admm_byte_model(const AdmmTables& T, bool fused, double coupling_bytes, const SellShape& hang, const SellShape& gamma,
                          const SellShape& gamma1, int64_t ngam1, const std::vector<const FactItfShape*>& fact,
                          const SellShape& aux, const SellShape& lam, const SellShape& wv) {
    AdmmBytes B;
    double nu = 0.0, rows = 0.0;
    for (auto& S : T.subs) nu += 3.0 * (double)S.nn + (double)S.nh;
    for (auto& sd : T.sides) rows += (double)sd.m;
    double fine_nodes = 0.0;
    for (auto& S : T.subs) fine_nodes += (double)S.nn;
    // the coupling rows; consForc copied into b (16 B per dof), k_outp (x, presc read, u written,
    // mask, node map: 77 B per node), the hanging rows
    B.rhs += coupling_bytes;
    B.rhs += 16.0 * 3.0 * fine_nodes + 77.0 * fine_nodes + (T.NH ? hang.bytes : 0.0);
    // interface: gamma (stored rows + the constant), factored per-ip kernels, projection,
    // the aux / lambda right-hand sides, the fused update (or the lambda add)
    B.iface += gamma.nch ? gamma.bytes + 8.0 * (double)gamma.nrow : 0.0;
    // side-1 halves of rank-local interfaces: their rows, then gamma read + written and the half read
    B.iface += gamma1.nch ? gamma1.bytes + 28.0 * (double)ngam1 : 0.0;
    for (const FactItfShape* F : fact) B.iface += F->bytes_gamma + (fused ? F->bytes_inpo : 0.0);
    for (auto& I : T.itfs)
        if (I.mine) B.iface += (double)(I.mip / I.comp) * (16.0 * I.comp + 4.0) + (I.cross ? 24.0 * I.mip : 0.0);
    if (fused) B.iface += wv.bytes + 56.0 * rows;
    else if (!T.sides.empty()) B.iface += aux.bytes + lam.bytes + 24.0 * rows;
    // MONITOR: snapshots of u and [aux, lambda] (read + written), the pair norms (16 B per entry)
    B.moni = 16.0 * (nu + 2.0 * rows) + 16.0 * (nu + 2.0 * rows);
    return B;
}

// ------------------------------------------------------------------------------- coarse right-hand side
int64_t CoarseSlots::slot_of(int64_t r, int64_t tv) const {
    const auto& v = srcs[r];
    const auto it = std::lower_bound(v.begin(), v.end(), tv);
    if (it == v.end() || *it != tv)
        throw ApiError(DDPCA_EINVAL, "coarse right-hand side: row " + std::to_string(r) + " has an entry of subdomain " +
                                         std::to_string(tv) + ", which is not on the row's interface graph");
    return sptr[r] + (int64_t)(it - v.begin());
}

// Row r of the coarse right-hand side sums contributions of several subdomains (its own u and
// lambda, its interface mates' through globTran_1 / globTran_S; LATIN's contact rows both bodies of
// the interface), and every source subdomain lives on exactly one rank.  Summing the row over this
// rank's W columns and then all-reducing across ranks would round differently for every rank
// layout; instead every row has one slot per structurally possible source (the same layout on
// every rank: itself and its interface mates, for LATIN's contact rows both bodies), each slot is
// summed in a fixed, layout-independent order by its source's owner (the other ranks contribute
// exact zeros to it), the slots are all-reduced, and k_slot_sum adds a row's slots in ascending
// source order.  The coarse right-hand side -- and so the whole trajectory -- is then the same
// bits on any number of ranks (tests/test_mcontact_gpu.py: resuMoni rows of the multi-rank runs;
// tests/sanitize/host_driver.cpp compares the plans of one and two ranks slot by slot).
CoarseRhsPlan plan_coarse_rhs(const MCONTACT& mc, const AdmmTables& T) {
    const CoarseSpace& cs = mc.coarse;
    CoarseRhsPlan C;
    const int64_t n = cs.n;
    C.xoff.resize(T.subs.size());
    for (size_t i = 0; i < T.subs.size(); ++i) {
        const int64_t tv = T.subs[i].tv;
        if (!cs.built[tv]) throw ApiError(DDPCA_ESTATE, "coarse rows of an owned subdomain were not built");
        C.xoff[i] = (int64_t)C.own_rows.size();
        for (int64_t r = cs.baseReco[tv]; r < cs.baseReco[tv + 1]; ++r) C.own_rows.push_back(r);
    }
    const int64_t nsg = (int64_t)cs.baseReco.size() - 1, nbase = cs.baseReco.back();
    auto& srcs = C.slots.srcs;
    srcs.resize(n);
    {
        std::vector<std::vector<int64_t>> nbr(nsg);
        std::vector<int64_t> bodies;
        for (int64_t tv = 0; tv < nsg; ++tv) nbr[tv].push_back(tv);
        for (const auto& itf : mc.searCont) {
            nbr[itf.body[0]].push_back(itf.body[1]);
            nbr[itf.body[1]].push_back(itf.body[0]);
            bodies.push_back(itf.body[0]);
            bodies.push_back(itf.body[1]);
        }
        auto uniq = [](std::vector<int64_t>& v) {
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
        };
        for (auto& v : nbr) uniq(v);
        uniq(bodies);
        for (int64_t tv = 0; tv < nsg; ++tv)
            for (int64_t r = cs.baseReco[tv]; r < cs.baseReco[tv + 1]; ++r) srcs[r] = nbr[tv];
        // LATIN's coarse contact unknowns: rows of interface ts take its two bodies when the
        // unknowns are known per interface (coarNode), else every body of an interface
        int64_t known = 0;
        for (int64_t ts = 0; ts < (int64_t)cs.coarNode.size(); ++ts)
            known += mc.searCont[ts].comp() * (int64_t)cs.coarNode[ts].size();
        if (cs.coarNode.size() == mc.searCont.size() && nbase + known == n) {
            int64_t r = nbase;
            for (int64_t ts = 0; ts < (int64_t)cs.coarNode.size(); ++ts) {
                std::vector<int64_t> b{mc.searCont[ts].body[0], mc.searCont[ts].body[1]};
                uniq(b);
                for (int64_t q = 0; q < mc.searCont[ts].comp() * (int64_t)cs.coarNode[ts].size(); ++q) srcs[r++] = b;
            }
        } else {
            for (int64_t r = nbase; r < n; ++r) srcs[r] = bodies;
        }
    }
    auto& sptr = C.slots.sptr;
    sptr.assign(n + 1, 0);
    for (int64_t r = 0; r < n; ++r) sptr[r + 1] = sptr[r] + (int64_t)srcs[r].size();
    C.nslot = sptr[n];
    // RHS entries over W: + globTran_1 (owned sides, lambda columns), - interface part of
    // globTran_D_1 (owned subdomains, u columns); LATIN + globTran lambda - globTran_pena aux +
    // globTran_D u.  Sort key inside a slot: (segment, global side, column in the source's own
    // numbering) -- none of it depends on where the source's columns sit in this rank's W
    struct Ent {
        int64_t seg, side, lcol;
        int32_t wc;
        double v;
        bool operator<(const Ent& o) const {
            return seg != o.seg ? seg < o.seg : side != o.side ? side < o.side : lcol < o.lcol;
        }
    };
    std::vector<std::vector<Ent>> ents(C.nslot);
    auto put = [&](int64_t r, int64_t tv, Ent e) { ents[C.slots.slot_of(r, tv)].push_back(e); };
    for (const auto& sd : T.sides) {
        const int64_t lam0 = T.oS + T.R + sd.roff, aux0 = T.oS + sd.roff, sg = 2 * sd.ts + sd.s;
        const auto& Su = T.subs[sd.sub];
        auto add_rows = [&](const Csr& A, int64_t seg, int64_t c0, double sgn, bool ucol) {
            for (int64_t r = 0; r < A.nrow; ++r)
                for (int64_t k = A.ptr[r]; k < A.ptr[r + 1]; ++k)
                    put(r, sd.tv, Ent{seg, sg, A.col[k], w32(ucol ? Su.wcol(A.col[k], T.oH) : c0 + A.col[k]), sgn * A.val[k]});
        };
        if (cs.latin) {  // (MCONTACT.h:2540-2548)
            add_rows(cs.globTran_D_L[sd.ts][sd.s], 1, 0, 1.0, true);
            add_rows(cs.globTran_pena_L[sd.ts][sd.s], 2, aux0, -1.0, false);
            add_rows(cs.globTran_L[sd.ts][sd.s], 3, lam0, 1.0, false);
        } else {
            add_rows(cs.globTran_1[sd.ts][sd.s], 3, lam0, 1.0, false);
        }
    }
    for (size_t i = 0; i < T.subs.size() && !cs.latin; ++i) {
        // factored: the interface part (the stiffness part is the SpMV + restriction chain);
        // assembled: the caller's whole globTran_D_1
        const Csr& A = cs.assembled ? cs.globTran_D_full[T.subs[i].tv] : cs.globTran_S[T.subs[i].tv];
        const auto& Su = T.subs[i];
        for (int64_t r = 0; r < A.nrow; ++r)
            for (int64_t k = A.ptr[r]; k < A.ptr[r + 1]; ++k)
                put(r, Su.tv, Ent{0, 0, A.col[k], w32(Su.wcol(A.col[k], T.oH)), -A.val[k]});
    }
    C.rptr.assign(C.nslot + 1, 0);
    for (int64_t q = 0; q < C.nslot; ++q) {
        auto& e = ents[q];
        std::stable_sort(e.begin(), e.end());
        for (const auto& x : e) {
            C.rcol.push_back(x.wc);
            C.rval.push_back(x.v);
        }
        C.rptr[q + 1] = (int64_t)C.rcol.size();
        std::vector<Ent>().swap(e);
    }
    // right-hand side CSR over W: entries, each distinct W entry once, f0 read and the slot
    // written; the slot sum reads the slots and row pointers and writes g
    C.bytes = 12.0 * (double)C.rcol.size() + 8.0 * (double)count_distinct(C.rcol) + 16.0 * (double)C.nslot +
              8.0 * (double)C.nslot + 16.0 * (double)n;
    if (C.rcol.empty()) {  // (never an empty device buffer)
        C.rcol.assign(1, 0);
        C.rval.assign(1, 0.0);
    }
    // globForc_1 enters the slot of the row's own subdomain (the rank that owns the row)
    C.f0.assign(std::max<int64_t>(C.nslot, 1), 0.0);
    for (size_t i = 0; i < T.subs.size(); ++i)
        for (int64_t r = cs.baseReco[T.subs[i].tv]; r < cs.baseReco[T.subs[i].tv + 1]; ++r)
            C.f0[C.slots.slot_of(r, T.subs[i].tv)] = cs.globForc_1[r];
    return C;
}

// The reference solves globCoup_1 directly below DIRE_MAXI = 120000 rows and with its DOUBLE_M_1
// MGPIS above (PREP.h:69, MCONTACT.h:1857-1865); the tuning's coarse_mg_min moves the switch
// (tests).  The direct solve here is a dense explicit inverse, n^2 8 B on every rank and streamed
// by the GEMV every ADMM iteration, so it is also bounded by memory: above coarse_dense_mb
// (default 1024 MiB, n ~ 11,600 rows) the multigrid solve takes over below DIRE_MAXI too -- where
// the inverse would cost ~0.2 ms of HBM streaming per iteration and grow as n^2
CoarseSolveChoice coarse_solve_choice(const CoarseSpace& cs, int64_t nown, int nranks, const AdmmTuning& tune) {
    CoarseSolveChoice S;
    const int64_t n = cs.n;
    const double dense_max = tune.coarse_dense_mb * 1048576.0;
    S.dense_bytes = 8.0 * (double)n * (double)n;
    const bool by_rows = n >= tune.coarse_mg_min;
    const bool by_budget = S.dense_bytes > dense_max;  // the same decision on every rank: n is global
    // LATIN: DOUBLE_M (MCONTACT.h:1236) on the coarse contact nodes (the host MULTISCALE's, or the
    // caller's through ddpca_problem_set_coarse_nodes)
    if (cs.latin && cs.coarNode.empty() && (by_rows || by_budget))
        throw ApiError(DDPCA_EINVAL, "LATIN coarse space past the dense solve's limits needs its coarse contact nodes "
                                     "(ddpca_problem_set_coarse_nodes) for DOUBLE_M");
    S.mg = by_rows || by_budget;
    // the multigrid hierarchy needs the whole coarse operator: a caller's full operator or a
    // single-rank build has it; a rank-local build gathers it from every rank once the transport
    // exists (coarse_invert)
    bool full = !cs.rank_local;
    for (int64_t tv = 0; tv < (int64_t)cs.built.size(); ++tv) full = full && cs.built[tv];
    if (S.mg && !full && nranks == 1)
        throw ApiError(DDPCA_ESTATE, "DOUBLE_M coarse solve: a single rank without every subdomain's coarse rows");
    S.mg_gather = S.mg && !full;
    // the owned rows of the dense inverse against g, or (DOUBLE_M) g scattered into the coarse
    // MGPIS and its owned rows gathered back (its PCG is counted by its own model)
    S.bytes = S.mg ? 20.0 * (double)n + 24.0 * (double)nown : 8.0 * (double)nown * (double)n + 8.0 * (double)n + 8.0 * (double)nown;
    return S;
}

std::vector<double> coarse_dense_rows(const CoarseSpace& cs, const std::vector<int64_t>& own_rows, int rank) {
    const int64_t n = cs.n;
    std::vector<double> dense((size_t)n * n, 0.0);
    std::vector<int64_t> fill_rows = own_rows;
    // the coarse contact unknowns' rows: a caller's full operator is filled by rank 0 only; a
    // rank-local host build holds each rank's share (the all-reduce sums them)
    if (cs.latin && (cs.rank_local || rank == 0))
        for (int64_t r = cs.baseReco.back(); r < n; ++r) fill_rows.push_back(r);
    for (int64_t r : fill_rows)
        for (int64_t k = cs.globCoup_1.ptr[r]; k < cs.globCoup_1.ptr[r + 1]; ++k)
            dense[(size_t)r * n + cs.globCoup_1.col[k]] = cs.globCoup_1.val[k];
    return dense;
}

// ---- DOUBLE_M_1 (MCONTACT.h:2303-2341): level l of the coarse hierarchy (l = Lc = max doleMcsc is
// globCoup_1 itself) holds level max(0, doleMcsc[tv] - (Lc - l)) of every subdomain; the transfer
// below it is each subdomain's realProl at that level (identity where a subdomain has reached its
// level 0), and the level operators are Galerkin products.  Nodes are numbered so that every level
// is a prefix of the next (the layout MgpisDevice takes): level l = level l-1's nodes, then the new
// nodes of every subdomain in order.  Needs every subdomain's coarse rows on this rank.
MgPlan plan_coarse_mg(const MCONTACT& mc, int64_t n) {
    const CoarseSpace& cs = mc.coarse;
    const int64_t nsub = (int64_t)mc.multGrid.size();
    MgPlan PL;
    const int64_t Lc = *std::max_element(mc.doleMcsc.begin(), mc.doleMcsc.end());
    auto lev = [&](int64_t tv, int64_t l) { return std::max<int64_t>(0, mc.doleMcsc[tv] - (Lc - l)); };
    std::vector<std::vector<std::vector<int64_t>>> gid(Lc + 1, std::vector<std::vector<int64_t>>(nsub));
    // LATIN (DOUBLE_M, MCONTACT.h:1538-1670): the coarse contact unknowns of every interface are a
    // group of their own -- at level Lc the level-doleMcsc nodes coarNode[ts] of contBody[ts][0],
    // one level down the columns its scalProl rows touch (ficoCotr), comp unknowns per node
    // (the node's first dof for frictionless contact).  The sets need not be nested: a node of
    // level l - 1 that level l does not carry (stacked bodies: BLOCK) keeps the prefix layout as a
    // masked copy on level l and above (per-level dof flags, SubdomainOps::dof_free_lev) -- the
    // masked transfer C_l P C_{l-1}^T then is the reference's ficoCotr
    const int64_t nint = cs.latin ? (int64_t)mc.searCont.size() : 0;
    if (cs.latin && (int64_t)cs.coarNode.size() != nint)
        throw ApiError(DDPCA_EINVAL, "DOUBLE_M for the LATIN coarse space needs the coarse contact nodes (coarNode)");
    std::vector<std::vector<std::vector<int64_t>>> cset(Lc + 1, std::vector<std::vector<int64_t>>(nint));
    for (int64_t ts = 0; ts < nint; ++ts) {
        const int64_t b0 = mc.searCont[ts].body[0];
        const MULTIGRID& g = mc.multGrid[b0];
        cset[Lc][ts] = cs.coarNode[ts];
        for (int64_t l = Lc; l >= 1; --l) {
            const int64_t fl = mc.doleMcsc[b0] - (Lc - l);  // the group's node level at l
            if (fl - 1 < 0) {
                cset[l - 1][ts] = cset[l][ts];
                continue;
            }
            const Stencil& Sp = g.scalProl[fl - 1];  // scalar, no rotations (MCONTACT.h:1553)
            if (!Sp.bent.empty())
                throw ApiError(DDPCA_EINVAL, "LATIN DOUBLE_M: ficoCotr needs the scalar scalProl (a caller's rotated realProl has none)");
            std::vector<int64_t> cols;
            for (int64_t f : cset[l][ts])
                for (int64_t k = Sp.ptr[f]; k < Sp.ptr[f + 1]; ++k) cols.push_back(Sp.col[k]);
            std::sort(cols.begin(), cols.end());
            cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
            cset[l - 1][ts] = cols;
        }
    }
    std::vector<std::unordered_map<int64_t, int64_t>> cg(nint);  // (interface, node) -> global node
    std::vector<int64_t> nglob(Lc + 1, 0);
    for (int64_t l = 0; l <= Lc; ++l) {
        int64_t cnt = l ? nglob[l - 1] : 0;
        for (int64_t tv = 0; tv < nsub; ++tv) {
            auto& v = gid[l][tv];
            v.resize(mc.multGrid[tv].leveCount[lev(tv, l)]);
            int64_t keep = 0;
            if (l) {
                keep = (int64_t)gid[l - 1][tv].size();
                std::copy(gid[l - 1][tv].begin(), gid[l - 1][tv].end(), v.begin());
            }
            for (int64_t j = keep; j < (int64_t)v.size(); ++j) v[j] = cnt++;
        }
        for (int64_t ts = 0; ts < nint; ++ts)
            for (int64_t node : cset[l][ts])
                if (cg[ts].emplace(node, cnt).second) ++cnt;
        nglob[l] = cnt;
    }
    std::vector<Stencil> S(Lc);
    for (int64_t l = 1; l <= Lc; ++l) {
        std::vector<std::vector<std::pair<int32_t, double>>> rows(nglob[l]);
        for (int64_t i = 0; i < nglob[l - 1]; ++i) rows[i].push_back({(int32_t)i, 1.0});
        std::vector<std::vector<std::array<double, 9>>> rblk(nglob[l]);  // block entries, parallel to rows (NaN-free marker below)
        for (int64_t tv = 0; tv < nsub; ++tv) {
            if (lev(tv, l) == lev(tv, l - 1)) continue;  // identity (MCONTACT.h:2325-2331)
            // the subdomain's realProl at that level (MCONTACT.h:1632, 2316): prolOper's rotation
            // blocks as block entries (a caller's operator-level stencil carries them in scalProl)
            const MULTIGRID& g = mc.multGrid[tv];
            const Stencil& Sp = g.prolOper.empty() ? g.scalProl[lev(tv, l - 1)] : g.prolOper[lev(tv, l - 1)];
            std::vector<int64_t> bo(Sp.col.size(), -1);
            for (size_t q = 0; q < Sp.bent.size(); ++q) bo[Sp.bent[q]] = (int64_t)q;
            for (int64_t j = (int64_t)gid[l - 1][tv].size(); j < (int64_t)gid[l][tv].size(); ++j)
                for (int64_t k = Sp.ptr[j]; k < Sp.ptr[j + 1]; ++k) {
                    const int64_t r = gid[l][tv][j];
                    rows[r].push_back({(int32_t)gid[l - 1][tv][Sp.col[k]], Sp.w[k]});
                    std::array<double, 9> b;
                    if (bo[k] >= 0) std::copy(&Sp.bval[9 * bo[k]], &Sp.bval[9 * bo[k]] + 9, b.begin());
                    else b[0] = std::numeric_limits<double>::quiet_NaN();  // scalar entry
                    rblk[r].resize(rows[r].size());
                    rblk[r].back() = b;
                }
        }
        for (int64_t ts = 0; ts < nint; ++ts) {  // ficoCotr rows of the nodes new on level l
            const int64_t b0 = mc.searCont[ts].body[0];
            const int64_t fl = mc.doleMcsc[b0] - (Lc - l);
            if (fl - 1 < 0) continue;
            const Stencil& Sp = mc.multGrid[b0].scalProl[fl - 1];
            for (int64_t f : cset[l][ts]) {
                if (std::binary_search(cset[l - 1][ts].begin(), cset[l - 1][ts].end(), f)) continue;  // coarse copy
                auto& row = rows[cg[ts].at(f)];
                for (int64_t k = Sp.ptr[f]; k < Sp.ptr[f + 1]; ++k) row.push_back({(int32_t)cg[ts].at(Sp.col[k]), Sp.w[k]});
            }
        }
        Stencil& Tr = S[l - 1];
        Tr.nf = nglob[l];
        Tr.nc = nglob[l - 1];
        Tr.ptr.assign(1, 0);
        for (int64_t r = 0; r < nglob[l]; ++r) {
            for (size_t q = 0; q < rows[r].size(); ++q) {
                const bool blk = q < rblk[r].size() && !std::isnan(rblk[r][q][0]);
                if (blk) {
                    Tr.bent.push_back((int64_t)Tr.col.size());
                    Tr.bval.insert(Tr.bval.end(), rblk[r][q].begin(), rblk[r][q].end());
                }
                Tr.col.push_back(rows[r][q].first);
                Tr.w.push_back(blk ? 0.0 : rows[r][q].second);
            }
            Tr.ptr.push_back((int64_t)Tr.col.size());
        }
    }
    // globCoup(_1) rows: subdomain tv's level-doleMcsc free dofs in increasing order (consOper),
    // then (LATIN) every interface's coarse contact unknowns, comp per node
    std::vector<int32_t> fdg(n);
    for (int64_t tv = 0; tv < nsub; ++tv) {
        const MULTIGRID& g = mc.multGrid[tv];
        int64_t r = cs.baseReco[tv];
        for (int64_t dof = 0; dof < 3 * g.leveCount[mc.doleMcsc[tv]]; ++dof)
            if (g.consFlag[dof]) {
                if (r >= cs.baseReco[tv + 1]) throw ApiError(DDPCA_EINVAL, "DOUBLE_M: baseReco does not match the free dofs");
                fdg[r++] = (int32_t)(3 * gid[Lc][tv][dof / 3] + dof % 3);
            }
        if (r != cs.baseReco[tv + 1]) throw ApiError(DDPCA_EINVAL, "DOUBLE_M: baseReco does not match the free dofs");
    }
    {
        int64_t r = cs.baseReco[nsub];
        for (int64_t ts = 0; ts < nint; ++ts) {
            const int comp = mc.searCont[ts].comp();
            for (int64_t node : cset[Lc][ts])
                for (int j = 0; j < comp; ++j) {
                    if (r >= n) throw ApiError(DDPCA_EINVAL, "DOUBLE_M: coarse contact unknowns do not match the coarse rows");
                    fdg[r++] = (int32_t)(3 * cg[ts].at(node) + j);
                }
        }
        if (r != n) throw ApiError(DDPCA_EINVAL, "DOUBLE_M: coarse contact unknowns do not match the coarse rows");
    }
    // per-level dof flags: a subdomain node's dofs as its consOper (the prefix of its flags), a
    // contact unknown's comp dofs free on the levels that carry it, its masked copies none
    std::vector<std::vector<uint8_t>> flev(Lc + 1);
    for (int64_t l = 0; l <= Lc; ++l) {
        auto& f = flev[l];
        f.assign(3 * nglob[l], 0);
        for (int64_t tv = 0; tv < nsub; ++tv) {
            const MULTIGRID& g = mc.multGrid[tv];
            for (size_t j = 0; j < gid[l][tv].size(); ++j)
                for (int a = 0; a < 3; ++a) f[3 * gid[l][tv][j] + a] = g.consFlag[3 * j + a];
        }
        for (int64_t ts = 0; ts < nint; ++ts) {
            const int comp = mc.searCont[ts].comp();
            for (int64_t node : cset[l][ts])
                for (int j = 0; j < comp; ++j) f[3 * cg[ts].at(node) + j] = 1;
        }
    }
    for (int32_t d : fdg)
        if (!flev[Lc][d]) throw ApiError(DDPCA_EINVAL, "DOUBLE_M: a coarse row on a constrained dof");
    PL.nglob = std::move(nglob);
    PL.S = std::move(S);
    PL.fdg = std::move(fdg);
    PL.flev = std::move(flev);
    PL.latin = cs.latin;
    return PL;
}

// ------------------------------------------------------------------------------- prolongation
CoarseProlongPlan plan_prolong_assembled(const MCONTACT& mc, const AdmmTables& T, const std::vector<int64_t>& xoff) {
    const CoarseSpace& cs = mc.coarse;
    CoarseProlongPlan C;
    C.pptr.assign(1, 0);
    for (size_t i = 0; i < T.subs.size(); ++i) {
        const int64_t tv = T.subs[i].tv;
        const MULTIGRID& g = mc.multGrid[tv];
        const Csr& A = cs.accuProl_full[tv];
        std::vector<int64_t> f2d(g.freeCount.back(), -1);
        for (int64_t d = 0; d < 3 * g.leveCount.back(); ++d)  // the fine level (not the hanging one)
            if (g.freeIndex[d] >= 0) f2d[g.freeIndex[d]] = d;
            else C.cdof.push_back(w32(T.subs[i].dof0 + d));
        for (int64_t r = 0; r < A.nrow; ++r) {
            for (int64_t k = A.ptr[r]; k < A.ptr[r + 1]; ++k) {
                C.pcol.push_back((int32_t)(xoff[i] + A.col[k]));
                C.pval.push_back(A.val[k]);
            }
            C.pptr.push_back((int64_t)C.pcol.size());
            C.ptgt.push_back(w32(T.subs[i].dof0 + f2d[r]));
        }
    }
    C.npr = (int64_t)C.ptgt.size();
    C.ncd = (int64_t)C.cdof.size();
    // u += accuProl x_c on the free rows (entries, target index, u read + written), the
    // constrained rows' prescribed values again
    C.bytes = 12.0 * (double)C.pcol.size() + 20.0 * (double)C.npr + 28.0 * (double)C.ncd;
    // (never an empty device buffer)
    if (C.pcol.empty()) C.pcol.assign(1, 0), C.pval.assign(1, 0.0);
    if (C.ptgt.empty()) C.ptgt.assign(1, 0);
    if (C.cdof.empty()) C.cdof.assign(1, 0);
    return C;
}

CoarseProlongPlan plan_prolong_factored(const MCONTACT& mc, const AdmmTables& T, const BatchView& V, const CoarseSlots& slots,
                                        const std::vector<int64_t>& xoff) {
    const CoarseSpace& cs = mc.coarse;
    CoarseProlongPlan C;
    const int L = (int)V.lev.size() - 1;
    // stiffness part: gather level-d device values into the owned coarse rows
    C.dmin = L;
    std::map<int, KGroupPlan> groups;
    std::vector<int64_t> xnoff(T.subs.size(), 0);
    int64_t nxn = 0;
    for (size_t i = 0; i < T.subs.size(); ++i) {
        const int64_t tv = T.subs[i].tv;
        const MULTIGRID& g = mc.multGrid[tv];
        const int d = (int)mc.doleMcsc[tv];
        if (g.maxiLeve != L) throw ApiError(DDPCA_EINVAL, "batched subdomains need equal level counts");
        C.dmin = std::min(C.dmin, d);
        auto& grp = groups[d];
        grp.level = d;
        const auto& perm = (*V.level_perm)[d][i];
        for (int64_t dof = 0; dof < 3 * g.leveCount[d]; ++dof) {
            const int32_t fi = g.freeIndex[dof];
            if (fi < 0) continue;
            grp.rows.push_back(w32(slots.slot_of(cs.baseReco[tv] + fi, tv)));  // the row's own slot
            grp.src.push_back(3 * (V.lev[d].noff[i] + perm[dof / 3]) + dof % 3);
        }
        xnoff[i] = nxn;
        nxn += 3 * g.leveCount[d];
    }
    double krows = 0.0;
    for (auto& kv : groups) {
        krows += (double)kv.second.rows.size();
        C.kg.push_back(std::move(kv.second));
    }
    // xn <- xc, and the accumulated prolongation (fine node -> level-d node) per batch node
    C.nxn = nxn;
    C.xsrc.assign(std::max<int64_t>(nxn, 1), -1);
    C.qnn = V.lev.back().nn;
    C.qcol.assign(8 * C.qnn, -1);
    C.qw.assign(8 * C.qnn, 0.0);
    C.flag.assign(T.NU, 0);
    C.pptr.assign(1, 0);
    for (size_t i = 0; i < T.subs.size(); ++i) {
        const int64_t tv = T.subs[i].tv;
        const MULTIGRID& g = mc.multGrid[tv];
        const int d = (int)mc.doleMcsc[tv];
        for (int64_t dof = 0; dof < 3 * g.leveCount[d]; ++dof) {
            const int32_t fi = g.freeIndex[dof];
            C.xsrc[xnoff[i] + dof] = fi < 0 ? -1 : (int32_t)(xoff[i] + fi);
        }
        const Stencil& Q = cs.accuQ[tv];
        const int64_t b0 = T.subs[i].dof0 / 3;
        std::vector<int64_t> bo(Q.col.size(), -1);
        for (size_t q = 0; q < Q.bent.size(); ++q) bo[Q.bent[q]] = (int64_t)q;
        for (int64_t nd = 0; nd < Q.nf; ++nd) {
            const int64_t len = Q.ptr[nd + 1] - Q.ptr[nd];
            bool scalar = len <= 8;
            for (int64_t k = Q.ptr[nd]; k < Q.ptr[nd + 1] && scalar; ++k) scalar = bo[k] < 0;
            if (scalar) {
                for (int64_t k = 0; k < len; ++k) {
                    C.qcol[k * C.qnn + b0 + nd] = (int32_t)(xnoff[i] + 3 * Q.col[Q.ptr[nd] + k]);
                    C.qw[k * C.qnn + b0 + nd] = Q.w[Q.ptr[nd] + k];
                }
                continue;
            }
            // a CSR row per free dof over x_c (the scalar kernel adds 0 there and the prescribed
            // values of the node's constrained dofs)
            for (int a = 0; a < 3; ++a) {
                const int64_t dof = 3 * nd + a;
                if (!g.consFlag[dof]) continue;
                for (int64_t k = Q.ptr[nd]; k < Q.ptr[nd + 1]; ++k) {
                    const int64_t c = Q.col[k];
                    for (int b = 0; b < 3; ++b) {
                        if (bo[k] < 0 && b != a) continue;
                        const int32_t f = g.freeIndex[3 * c + b];
                        const double w = bo[k] < 0 ? Q.w[k] : Q.bval[9 * bo[k] + 3 * a + b];
                        if (f < 0 || w == 0.0) continue;
                        C.pcol.push_back((int32_t)(xoff[i] + f));
                        C.pval.push_back(w);
                    }
                }
                C.pptr.push_back((int64_t)C.pcol.size());
                C.ptgt.push_back(w32(T.subs[i].dof0 + dof));
            }
        }
        for (int64_t dof = 0; dof < 3 * g.leveCount.back(); ++dof) C.flag[T.subs[i].dof0 + dof] = g.consFlag[dof];
    }
    C.npr = (int64_t)C.ptgt.size();
    C.ncd = 0;
    if (C.npr) {
        C.bytes_csr = 12.0 * (double)C.pcol.size() + 20.0 * (double)C.npr;
        if (C.pcol.empty()) C.pcol.assign(1, 0), C.pval.assign(1, 0.0);  // (never an empty device buffer)
    }
    // factored stiffness part and prolongation: K x = b - r (b, r read, the difference written:
    // 72 B per fine node), the plain restriction chain down to dmin (r_f once, mask + b_c per
    // coarse node, the lattice's child mask + fine copy or the stencil's index + weight), the
    // gather of level-d values into g, x_c scattered to nodal xn, and u += (Q (x) I3) xn: Q's
    // entries, flags, u read + written, xn once
    double nf = 0.0, qent = 0.0, kp = 0.0;
    for (size_t i = 0; i < T.subs.size(); ++i) {
        nf += (double)T.subs[i].nn;
        qent += (double)cs.accuQ[T.subs[i].tv].col.size();
        for (int l = L; l > C.dmin; --l) {
            const BatchLevelView& F = V.lev[l];
            kp += 24.0 * (double)F.nloc[i] + (25.0 + (F.lat ? 8.0 : 0.0)) * (double)V.lev[l - 1].nloc[i] +
                  (F.lat ? 0.0 : 12.0 * (double)F.tent_sub[i]);
        }
    }
    C.bytes = 72.0 * nf + kp + 36.0 * krows + 20.0 * (double)nxn + 12.0 * qent + 51.0 * nf + 8.0 * (double)nxn;
    return C;
}

}  // namespace ddpca
