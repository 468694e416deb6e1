// ASan + UBSan driver of the host stress recovery (ddpca-admm_amd/csrc/stress.cpp): a 2 x 2 x 2 box
// refined once uniformly, then the 8 children of element 0 refined locally through the C++ classes
// (MULTIGRID::REFINE: edge and face hanging nodes), a nodal rotation on every fifth node, then
// TRANSFER + PATCH, STRESS_PLAN and STRESS_RECOVERY on a constant-strain field (every node must
// carry D sym(A)) and on a smooth one.  A plain CPU executable linked to the instrumented objects
// of tests/sanitize/Makefile (tests/test_stress_sanitize.py builds and runs it); a sanitizer
// report aborts it.
#include <cmath>
#include <cstdio>
#include <set>
#include <vector>

#include "multigrid.hpp"

using namespace ddpca;

int main() {
    MULTIGRID g;
    const double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {1.0, 1.2, 0.9};
    const int64_t n[3] = {2, 2, 2};
    build_box(g, lo, hi, n, 1);
    std::set<int64_t> split;
    for (int64_t c : g.elemVect[0].children) {
        split.insert(c);
        g.elemVect[c].refiPatt = 0;
    }
    g.REFINE(split, {}, {});
    const int64_t N = g.numNodes();
    g.nodeLevel.assign(N, 0);
    g.nodeParents.assign(N, {});
    for (int64_t i = 0; i < N; i += 5) {
        const double a = 0.3 + 0.01 * (double)i, c = std::cos(a), s = std::sin(a);
        g.nodeRota.emplace(i, std::array<double, 9>{c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0});
    }
    g.mateElas = 110.0e9;
    g.matePois = 0.25;
    g.force_general = true;
    g.TRANSFER();
    const StressPlan& P = g.STRESS_PLAN();
    int failures = 0;
    if (g.hangMap.empty() || P.nnode != N || P.ptr.back() <= 8 * P.nleaf) ++failures;

    const double A[3][3] = {{1.0e-4, 0.4e-4, -0.3e-4}, {0.1e-4, -0.7e-4, 0.5e-4}, {0.6e-4, -0.2e-4, 0.9e-4}};
    const double lam = g.mateElas * g.matePois / (1.0 + g.matePois) / (1.0 - 2.0 * g.matePois);
    const double mu = g.mateElas / 2.0 / (1.0 + g.matePois);
    const double tr = A[0][0] + A[1][1] + A[2][2];
    const double want[6] = {lam * tr + 2.0 * mu * A[0][0], lam * tr + 2.0 * mu * A[1][1], lam * tr + 2.0 * mu * A[2][2],
                            mu * (A[0][1] + A[1][0]),      mu * (A[1][2] + A[2][1]),      mu * (A[2][0] + A[0][2])};
    std::vector<double> u(3 * N), stre(7 * N);
    for (int pass = 0; pass < 2; ++pass) {
        for (int64_t p = 0; p < N; ++p) {
            const auto& x = g.nodeCoor[p];
            double v[3];
            for (int a = 0; a < 3; ++a)
                v[a] = pass == 0 ? A[a][0] * x[0] + A[a][1] * x[1] + A[a][2] * x[2] + 1.0e-5
                                 : 1.0e-5 * std::sin(1.3 * x[0] + 0.2 * a) * std::cos(0.9 * x[1]) * std::sin(0.7 * x[2] + 0.4);
            const auto it = g.nodeRota.find(p);
            for (int a = 0; a < 3; ++a)
                u[3 * p + a] = it == g.nodeRota.end() ? v[a] : it->second[a] * v[0] + it->second[3 + a] * v[1] + it->second[6 + a] * v[2];
        }
        g.STRESS_RECOVERY(u.data(), stre.data());
        for (int64_t p = 0; p < N; ++p)
            for (int c = 0; c < 7; ++c) {
                if (!std::isfinite(stre[7 * p + c])) ++failures;
                if (pass == 0 && c < 6 && std::abs(stre[7 * p + c] - want[c]) > 1.0e-10 * std::abs(want[0])) ++failures;
            }
    }
    std::printf("{\"ok\": %s, \"failures\": %d}\n", failures ? "false" : "true", failures);
    return failures ? 1 : 0;
}
