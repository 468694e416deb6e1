// MULTIGRID::STRESS_RECOVERY (MULTIGRID.h:1316-1433) restated on the host: the plan the device
// kernels share (STRESS_PLAN) and the CPU anchor of the tests / the device < 0 path of
// ddpca_multigrid_stress (STRESS_RECOVERY, OpenMP over elements and over nodes).
//
//   * nodal displacements arrive in the solver's frame; a node of nodeRota gets R u (1318-1324)
//   * per leaf element (corner coordinates after PATCH): the 3x3x3 Gauss rule's stresses
//     sigma_g = D B u_e, F = sum w |J| N^T sigma^T, M = sum w |J| N^T N, nodal stresses M^-1 F
//     (1348-1372).  M is symmetric positive definite, so the 8x8 solve is a Gauss-Jordan
//     elimination without pivoting (the reference's fullPivLu solves the same system)
//   * contributions in the reference's order (1373-1408): element by element, row j to corner j;
//     then row j of a hanging corner to each of its parents (finoCono); then, for each of the 12
//     edges and 6 faces whose sorted corner set is a key of conoFino, the mean of those rows to
//     the hanging node
//   * a node's result is the arithmetic mean of its contributions (summed from zero in that
//     order), then sigma_eq; a node with no contribution gets 0 / 0 = NaN, as in the reference
#include <algorithm>
#include <cmath>
#include <mutex>
#include <stdexcept>
#include <unordered_map>

#include "multigrid.hpp"
#include "stress_elem.hpp"

namespace ddpca {

namespace {

// PREP.h hexaLine / hexaFace
const int kLine[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {0, 4}, {1, 5}, {2, 6}, {3, 7}, {4, 5}, {5, 6}, {6, 7}, {7, 4}};
const int kFace[6][4] = {{0, 3, 2, 1}, {4, 5, 6, 7}, {0, 4, 7, 3}, {1, 2, 6, 5}, {0, 1, 5, 4}, {3, 7, 6, 2}};

struct KeyHash {
    size_t operator()(const std::array<int64_t, 4>& k) const {
        uint64_t h = 1469598103934665603ull;
        for (int64_t v : k) h = (h ^ (uint64_t)v) * 1099511628211ull;
        return (size_t)h;
    }
};

std::mutex& plan_mutex() {
    static std::mutex m;
    return m;
}

// nodal stresses of one element: X, U the corners' coordinates and (rotated) displacements,
// se = M^-1 F, 8 x 6 row-major
void element_stress(const double (&X)[8][3], const double (&Ue)[8][3], double lam, double mu, double* se) {
    double C[8][3], U[8][3];
    for (int i = 0; i < 8; ++i)
        for (int c = 0; c < 3; ++c) C[i][c] = U[i][c] = 0.0;
    for (int k = 0; k < 8; ++k)
        for (int i = 0; i < 8; ++i)
            for (int c = 0; c < 3; ++c) {
                C[i][c] += stress::mode_sign(i, k) * X[k][c];
                U[i][c] += stress::mode_sign(i, k) * Ue[k][c];
            }
    for (int i = 0; i < 8; ++i)
        for (int c = 0; c < 3; ++c) C[i][c] *= 0.125, U[i][c] *= 0.125;
    double M[8][8] = {}, F[8][6] = {};
    for (int gi = 0; gi < 3; ++gi)
        for (int gj = 0; gj < 3; ++gj)
            for (int gk = 0; gk < 3; ++gk) {
                const double x = stress::gauss_pt(gi), y = stress::gauss_pt(gj), z = stress::gauss_pt(gk);
                double sig[6];
                const double det = stress::gauss_stress(C, U, x, y, z, lam, mu, sig);
                const double w = stress::gauss_wt(gi) * stress::gauss_wt(gj) * stress::gauss_wt(gk) * det;
                double N[8];
                for (int k = 0; k < 8; ++k) N[k] = stress::shape(stress::sgn_xi(k), stress::sgn_eta(k), stress::sgn_zeta(k), x, y, z);
                for (int j = 0; j < 8; ++j) {
                    const double wn = w * N[j];
                    for (int c = 0; c < 6; ++c) F[j][c] += wn * sig[c];
                    for (int k = 0; k < 8; ++k) M[j][k] += wn * N[k];
                }
            }
    for (int k = 0; k < 8; ++k) {
        const double rinv = 1.0 / M[k][k];
        double p[8], pf[6];
        for (int c = k + 1; c < 8; ++c) p[c] = M[k][c] * rinv;
        for (int c = 0; c < 6; ++c) pf[c] = F[k][c] * rinv;
        for (int j = 0; j < 8; ++j) {
            const double f = M[j][k];
            for (int c = k + 1; c < 8; ++c) M[j][c] = j == k ? p[c] : M[j][c] - f * p[c];
            for (int c = 0; c < 6; ++c) F[j][c] = j == k ? pf[c] : F[j][c] - f * pf[c];
        }
    }
    for (int j = 0; j < 8; ++j)
        for (int c = 0; c < 6; ++c) se[6 * j + c] = F[j][c];
}

}  // namespace

const StressPlan& MULTIGRID::STRESS_PLAN() {
    std::lock_guard<std::mutex> lock(plan_mutex());
    if (strePlan) return *strePlan;
    const int64_t N = numNodes();
    if (elemVect.empty() || N == 0) throw std::invalid_argument("STRESS_PLAN: the subdomain has no element tree");
    if (leveCount.empty() || nodalCount() != N) throw std::invalid_argument("STRESS_PLAN: TRANSFER has not run on this tree");
    auto P = std::make_shared<StressPlan>();
    P->nnode = N;
    for (const auto& e : elemVect) {
        if (!e.leaf()) continue;
        for (int64_t c : e.cornNode) {
            if (c < 0 || c >= N) throw std::invalid_argument("STRESS_PLAN: corner node out of range");
            P->corner.push_back((int32_t)c);
        }
    }
    P->nleaf = (int64_t)P->corner.size() / 8;
    if (P->nleaf >= (int64_t)1 << 31) throw std::invalid_argument("STRESS_PLAN: leaf elements must fit int32");
    // finoCono (hanging node -> parents; the first key of a node wins, as emplace does) and conoFino
    std::unordered_map<int64_t, const std::vector<int64_t>*> fino;
    std::unordered_map<std::array<int64_t, 4>, int64_t, KeyHash> cono;
    for (const auto& kv : hangMap) {
        if (kv.first.size() > 4) continue;  // no edge or face has that many corners (never a key here)
        fino.emplace(kv.second, &kv.first);
        std::array<int64_t, 4> k{-1, -1, -1, -1};
        std::copy(kv.first.begin(), kv.first.end(), k.begin());
        cono.emplace(k, kv.second);
    }
    // the contributions in the reference's order, counted, then filled
    auto visit = [&](auto&& emit) {
        for (int64_t l = 0; l < P->nleaf; ++l) {
            const int32_t* cn = &P->corner[8 * l];
            for (int j = 0; j < 8; ++j) emit(cn[j], l, 1u << j);
            if (fino.empty()) continue;
            for (int j = 0; j < 8; ++j) {
                const auto it = fino.find(cn[j]);
                if (it != fino.end())
                    for (int64_t p : *it->second) emit(p, l, 1u << j);
            }
            for (const auto& ln : kLine) {
                std::array<int64_t, 4> k{std::min(cn[ln[0]], cn[ln[1]]), std::max(cn[ln[0]], cn[ln[1]]), -1, -1};
                const auto it = cono.find(k);
                if (it != cono.end()) emit(it->second, l, 1u << ln[0] | 1u << ln[1]);
            }
            for (const auto& f : kFace) {
                std::array<int64_t, 4> k{cn[f[0]], cn[f[1]], cn[f[2]], cn[f[3]]};
                std::sort(k.begin(), k.end());
                const auto it = cono.find(k);
                if (it != cono.end()) emit(it->second, l, 1u << f[0] | 1u << f[1] | 1u << f[2] | 1u << f[3]);
            }
        }
    };
    P->ptr.assign(N + 1, 0);
    visit([&](int64_t node, int64_t, unsigned) { P->ptr[node + 1]++; });
    for (int64_t i = 0; i < N; ++i) P->ptr[i + 1] += P->ptr[i];
    P->leaf.resize(P->ptr[N]);
    P->mask.resize(P->ptr[N]);
    std::vector<int64_t> fill(P->ptr.begin(), P->ptr.end() - 1);
    visit([&](int64_t node, int64_t l, unsigned m) {
        P->leaf[fill[node]] = (int32_t)l;
        P->mask[fill[node]++] = (uint8_t)m;
    });
    P->rotIndex.assign(N, -1);
    for (const auto& kv : nodeRota) {
        if (kv.first < 0 || kv.first >= N) continue;
        P->rotIndex[kv.first] = (int32_t)(P->rot.size() / 9);
        P->rot.insert(P->rot.end(), kv.second.begin(), kv.second.end());
    }
    strePlan = std::move(P);
    return *strePlan;
}

void MULTIGRID::STRESS_RECOVERY(const double* u_nodal, double* stre7) {
    const StressPlan& P = STRESS_PLAN();
    const double lam = mateElas * matePois / (1.0 + matePois) / (1.0 - 2.0 * matePois);
    const double mu = mateElas / 2.0 / (1.0 + matePois);
    std::vector<double> se((size_t)48 * P.nleaf);
#pragma omp parallel for schedule(static)
    for (int64_t l = 0; l < P.nleaf; ++l) {
        double X[8][3], U[8][3];
        for (int k = 0; k < 8; ++k) {
            const int64_t n = P.corner[8 * l + k];
            const double* u = u_nodal + 3 * n;
            const int32_t r = P.rotIndex[n];
            for (int a = 0; a < 3; ++a) {
                X[k][a] = nodeCoor[n][a];
                const double* R = r < 0 ? nullptr : &P.rot[9 * (size_t)r + 3 * a];
                U[k][a] = R ? R[0] * u[0] + R[1] * u[1] + R[2] * u[2] : u[a];
            }
        }
        element_stress(X, U, lam, mu, &se[(size_t)48 * l]);
    }
#pragma omp parallel for schedule(static)
    for (int64_t n = 0; n < P.nnode; ++n) {
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t q = P.ptr[n]; q < P.ptr[n + 1]; ++q) {
            double m[6];
            stress::masked_mean(&se[(size_t)48 * P.leaf[q]], P.mask[q], m);
            for (int c = 0; c < 6; ++c) s[c] += m[c];
        }
        const double cnt = (double)(P.ptr[n + 1] - P.ptr[n]);
        for (int c = 0; c < 6; ++c) s[c] = s[c] / cnt;
        for (int c = 0; c < 6; ++c) stre7[7 * n + c] = s[c];
        stre7[7 * n + 6] = std::sqrt(stress::von_mises_sq(s));
    }
}

}  // namespace ddpca
