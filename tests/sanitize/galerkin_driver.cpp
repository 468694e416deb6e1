// ASan + UBSan driver of the host side of the device Galerkin chain (galerkin_pattern,
// ddpca-admm_amd/csrc/sparse.cpp, and MULTIGRID::galerkinChain in CONSTRAINT): the tree of
// stress_driver.cpp (hanging nodes, a nodal rotation on every fifth node), STIF_MATR, then CONSTRAINT
// twice: with galerkin_rap, and with a hook that walks galerkin_pattern's arrays the way k_rap does
// (device_galerkin.hip: per stored block its owner compares every triple's column with its own, the
// children, blocks and entries in the pattern's order), on the host.  The hook's pattern must be
// galerkin_rap's byte for byte and its values within 1e-13 of the level's largest entry.  A plain CPU
// executable linked to the instrumented objects of tests/sanitize/Makefile
// (tests/test_galerkin_sanitize.py builds and runs it); a sanitizer report aborts it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <set>
#include <vector>

#include "multigrid.hpp"

using namespace ddpca;

namespace {

void entry_block(const Stencil& S, const std::vector<int64_t>& blk_of, int64_t e, double B[9]) {
    if (blk_of[e] >= 0)
        for (int i = 0; i < 9; ++i) B[i] = S.bval[9 * blk_of[e] + i];
    else
        for (int i = 0; i < 9; ++i) B[i] = i % 4 == 0 ? S.w[e] : 0.0;
}

Bsr3 rap_on_pattern(const Bsr3& A, const Stencil& S) {
    GalerkinPattern G = galerkin_pattern(A, S);
    std::vector<int64_t> blk_of(S.col.size(), -1);
    for (size_t q = 0; q < S.bent.size(); ++q) blk_of[S.bent[q]] = (int64_t)q;
    Bsr3 C;
    C.nb = C.mb = S.nc;
    C.val.assign(9 * G.col.size(), 0.0);
    for (int64_t c1 = 0; c1 < S.nc; ++c1)
        for (int64_t mine = G.ptr[c1]; mine < G.ptr[c1 + 1]; ++mine) {
            double* acc = &C.val[9 * mine];
            for (int64_t t = G.tptr[c1]; t < G.tptr[c1 + 1]; ++t) {
                const int64_t f1 = G.tfine[t];
                double B1[9];
                entry_block(S, blk_of, G.tent[t], B1);
                for (int64_t k = A.ptr[f1]; k < A.ptr[f1 + 1]; ++k) {
                    const double* a = A.block(k);
                    double T[9];
                    for (int i = 0; i < 3; ++i)
                        for (int j = 0; j < 3; ++j) T[3 * i + j] = B1[i] * a[j] + B1[3 + i] * a[3 + j] + B1[6 + i] * a[6 + j];
                    for (int64_t s = S.ptr[A.col[k]]; s < S.ptr[A.col[k] + 1]; ++s) {
                        if (S.col[s] != G.col[mine]) continue;
                        double B2[9];
                        entry_block(S, blk_of, s, B2);
                        for (int i = 0; i < 3; ++i)
                            for (int j = 0; j < 3; ++j)
                                acc[3 * i + j] += T[3 * i] * B2[j] + T[3 * i + 1] * B2[3 + j] + T[3 * i + 2] * B2[6 + j];
                    }
                }
            }
        }
    C.ptr = std::move(G.ptr);
    C.col = std::move(G.col);
    return C;
}

}  // namespace

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
    g.force_general = true;
    g.TRANSFER();
    g.STIF_MATR();
    MULTIGRID h = g;
    g.CONSTRAINT();
    int products = 0, with_blocks = 0;
    h.galerkinChain = [&](const Bsr3& K, const std::vector<const Stencil*>& chain, std::vector<Bsr3>& out) {
        out.clear();
        for (const Stencil* S : chain) {
            out.push_back(rap_on_pattern(out.empty() ? K : out.back(), *S));
            ++products;
            if (!S->bent.empty()) ++with_blocks;
        }
    };
    h.CONSTRAINT();
    int failures = 0;
    if (!g.nodeAll || products != (int)g.maxiLeve + 1 || with_blocks == 0) ++failures;
    if (g.levelStif.size() != h.levelStif.size()) ++failures;
    double worst = 0.0;
    for (size_t l = 0; l < g.levelStif.size() && !failures; ++l) {
        const Bsr3 &a = g.levelStif[l], &b = h.levelStif[l];
        if (a.ptr != b.ptr || a.col != b.col || a.val.size() != b.val.size()) {
            ++failures;
            break;
        }
        double big = 0.0, err = 0.0;
        for (size_t q = 0; q < a.val.size(); ++q) {
            big = std::max(big, std::abs(a.val[q]));
            err = std::max(err, std::abs(a.val[q] - b.val[q]));
        }
        worst = std::max(worst, err / big);
        if (!(err <= 1.0e-13 * big)) ++failures;
    }
    if (g.consFlag != h.consFlag || g.freeCount != h.freeCount) ++failures;
    std::fprintf(stderr, "galerkin_driver: %d products (%d with block entries), worst %.3e of the largest entry\n", products,
                 with_blocks, worst);
    std::printf("{\"ok\": %s, \"failures\": %d}\n", failures ? "false" : "true", failures);
    return failures ? 1 : 0;
}
