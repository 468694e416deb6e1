// ASan + UBSan driver of the host side of the device mortar operators (mortar_plan, ddpca-admm_amd/
// csrc/mortar_plan.cpp, and the walk of the kernels' thread bodies, mortar_host.cpp with
// mortar_point.hpp): the shapes of tests/mortar_cases.py that reach every branch -- patch (2 x 2 faces
// against 4 x 4, 16 points per face pair), collapsed (node[s][2] == node[s][3]: duplicate terms, equal
// sort keys), fan130 (a contact node with 131 partners: three lane passes), rot01 (rotated contact
// nodes on both sides, and rotated nodes that are none) and empty -- restated in C++ with a seeded
// generator, for fric 0, 0.2 and -1.  Each is built by mortar_build_host and by Interface::BUILD and
// every member compared byte for byte.  A plain CPU executable linked to the instrumented objects of
// tests/sanitize/Makefile (tests/test_mortar_sanitize.py builds and runs it); a sanitizer report
// aborts it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "mortar_plan.hpp"

using namespace ddpca;

namespace {

struct Case {
    std::string name;
    int64_t nn[2] = {0, 0};
    std::vector<IntegralPoint> ip;
    NodeRota rot[2];
};

void rotation(std::mt19937_64& rng, std::array<double, 9>& R) {
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    double a[3] = {u(rng), u(rng), u(rng)}, b[3] = {u(rng), u(rng), u(rng)};
    const double na = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    for (double& x : a) x /= na;
    const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    for (int i = 0; i < 3; ++i) b[i] -= ab * a[i];
    const double nb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    for (double& x : b) x /= nb;
    const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    for (int i = 0; i < 3; ++i) R[i] = a[i], R[3 + i] = b[i], R[6 + i] = c[i];
}

// `per` points for each pair of faces, with seeded values: an orthonormal basis, positive shape
// values that sum to 1 per side, w > 0, gaps of both signs
void add_points(Case& c, std::mt19937_64& rng, const int64_t f0[4], const int64_t f1[4], int per) {
    std::uniform_real_distribution<double> u(0.05, 1.0), g(-1.0e-3, 1.0e-3);
    for (int k = 0; k < per; ++k) {
        IntegralPoint p;
        for (int a = 0; a < 4; ++a) p.node[0][a] = f0[a], p.node[1][a] = f1[a];
        for (int s = 0; s < 2; ++s) {
            double sum = 0.0;
            for (int a = 0; a < 4; ++a) sum += p.shap[s][a] = u(rng);
            for (int a = 0; a < 4; ++a) p.shap[s][a] /= sum;
        }
        std::array<double, 9> R;
        rotation(rng, R);
        std::memcpy(p.basis, R.data(), sizeof p.basis);
        p.gap = g(rng);
        p.w = u(rng) * 1.0e-4;
        c.ip.push_back(p);
    }
}

void face(int n, int i, int j, int64_t f[4]) {
    const int64_t a = (int64_t)i * (n + 1) + j;
    f[0] = a, f[1] = a + n + 1, f[2] = a + n + 2, f[3] = a + 1;
}

Case patch(const char* name, unsigned seed) {
    Case c;
    c.name = name;
    c.nn[0] = 12, c.nn[1] = 30;
    std::mt19937_64 rng(seed);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            int64_t f0[4], f1[4];
            face(2, i / 2, j / 2, f0);
            face(4, i, j, f1);
            add_points(c, rng, f0, f1, 16);
        }
    return c;
}

Case collapsed() {
    Case c = patch("collapsed", 2);
    for (size_t q = 0; q < c.ip.size(); q += 2) c.ip[q].node[0][3] = c.ip[q].node[0][2];
    for (size_t q = 5; q < c.ip.size(); q += 7) c.ip[q].node[1][3] = c.ip[q].node[1][2];
    return c;
}

Case fan130() {
    Case c;
    c.name = "fan130";
    const int nf = 130;
    c.nn[0] = nf + 1, c.nn[1] = 11;
    std::mt19937_64 rng(4);
    for (int i = 0; i < nf; ++i) {
        const int64_t f0[4] = {0, 1 + i % nf, 1 + (i + 1) % nf, 1 + (i + 2) % nf};
        const int64_t f1[4] = {(3 * i) % 11, (3 * i + 1) % 11, (3 * i + 5) % 11, (3 * i + 7) % 11};
        add_points(c, rng, f0, f1, 2);
    }
    return c;
}

Case rot01() {
    Case c = patch("rot01", 8);
    std::mt19937_64 rng(9);
    for (int s = 0; s < 2; ++s) {
        std::vector<int64_t> cont;
        for (const auto& p : c.ip)
            for (int a = 0; a < 4; ++a) {
                bool seen = false;
                for (int64_t n : cont) seen = seen || n == p.node[s][a];
                if (!seen) cont.push_back(p.node[s][a]);
            }
        for (size_t k = 0; k < cont.size(); k += 3) rotation(rng, c.rot[s][cont[k]]);
        rotation(rng, c.rot[s][c.nn[s] - 1]);  // rotated nodes that are no contact nodes
        rotation(rng, c.rot[s][c.nn[s] - 2]);
    }
    return c;
}

Case empty() {
    Case c;
    c.name = "empty";
    c.nn[0] = 4, c.nn[1] = 5;
    return c;
}

template <typename T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
bool same(const Csr& a, const Csr& b) {
    return a.nrow == b.nrow && a.ncol == b.ncol && same(a.ptr, b.ptr) && same(a.col, b.col) && same(a.val, b.val);
}

int compare(const Interface& a, const Interface& b) {
    int bad = 0;
    for (int s = 0; s < 2; ++s) {
        bad += !same(a.nodeCont[s], b.nodeCont[s]);
        bad += !same(a.systMass[s], b.systMass[s]) + !same(a.systTran[s], b.systTran[s]) + !same(a.systTran_pena[s], b.systTran_pena[s]);
        bad += !same(a.inteMass[s], b.inteMass[s]) + !same(a.inteMass_pena[s], b.inteMass_pena[s]);
        bad += !same(a.inpoLagr[s], b.inpoLagr[s]) + !same(a.inpoDisp[s], b.inpoDisp[s]) + !same(a.inteInpo[s], b.inteInpo[s]);
        bad += !same(a.pemaInpo_r[s], b.pemaInpo_r[s]);
    }
    bad += !same(a.inpoNgap, b.inpoNgap) + !same(a.pemaDiag, b.pemaDiag) + (a.factored != b.factored);
    return bad;
}

}  // namespace

int main() {
    int failures = 0, builds = 0;
    const Case cases[] = {patch("patch", 2), collapsed(), fan130(), rot01(), empty()};
    for (const Case& c : cases)
        for (double fric : {0.0, 0.2, -1.0}) {
            Interface ref, out;
            for (Interface* itf : {&ref, &out}) {
                itf->ip = c.ip;
                itf->fric = fric;
                itf->penN = 3.0e9;
                itf->penF = 7.0e8;
            }
            const NodeRota* const rot[2] = {&c.rot[0], &c.rot[1]};
            ref.BUILD(c.nn, rot);
            mortar_build_host(mortar_input(out, c.nn, rot), out);
            const int bad = compare(ref, out);
            if (c.name == "rot01" ? ref.factored : !ref.factored) ++failures;
            if (c.name == "fan130" && ref.inteMass[0].ptr[1] != (int64_t)131 * ref.comp()) ++failures;
            if (bad) std::fprintf(stderr, "mortar_driver: %s fric %g: %d members differ\n", c.name.c_str(), fric, bad);
            failures += bad;
            ++builds;
        }
    // a node id outside [0, nn) is refused by the plan
    {
        Case c = patch("patch", 2);
        c.ip[3].node[1][2] = c.nn[1];
        Interface itf;
        itf.ip = c.ip;
        itf.fric = 0.2;
        const NodeRota* const rot[2] = {nullptr, nullptr};
        bool refused = false;
        try {
            mortar_build_host(mortar_input(itf, c.nn, rot), itf);
        } catch (const std::exception&) {
            refused = true;
        }
        if (!refused) ++failures;
    }
    std::fprintf(stderr, "mortar_driver: %d builds compared with Interface::BUILD\n", builds);
    std::printf("{\"ok\": %s, \"failures\": %d}\n", failures ? "false" : "true", failures);
    return failures ? 1 : 0;
}
