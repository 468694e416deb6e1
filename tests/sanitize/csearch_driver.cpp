// ASan + UBSan driver of the two-pass contact search (csearch.cpp: csearch_plan,
// csearch_two_pass_host, refine_flags, with the face arithmetic of csearch_face.hpp): a plain CPU
// executable with its own main, linked to the instrumented host objects of tests/sanitize/Makefile.
// It runs what ddpca_contact_search_on / ddpca_refine_select_on run for device = -2 -- everything the
// device path does but the launch -- on the inputs of tests/csearch_cases.py (coincident 8 x 8 flat
// faces: the degenerate clip with its list of 22; curved 12 x 12 against rotated 15 x 15: the stepped
// projection, empty intersections, clamped neighbourhoods) and on the refusals, and checks counts
// against the host search.  A sanitizer report aborts it.
#include <cmath>
#include <cstdio>
#include <functional>
#include <vector>

#include "../../include/ddpca_amd.h"
#include "common.hpp"
#include "device_csearch.hpp"

using namespace ddpca;

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

struct Side {
    std::vector<double> xyz, c2;
    std::vector<int64_t> faces;
};

Side grid(int n, const std::function<void(double, double, double*)>& xy) {
    Side s;
    for (int i = 0; i <= n; ++i)
        for (int j = 0; j <= n; ++j) {
            double p[3];
            xy((double)i / n, (double)j / n, p);
            s.xyz.insert(s.xyz.end(), p, p + 3);
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const int64_t a = (int64_t)i * (n + 1) + j, f[4] = {a, a + n + 1, a + n + 2, a + 1};
            s.faces.insert(s.faces.end(), f, f + 4);
            double c[2] = {0.0, 0.0};
            for (int k = 0; k < 4; ++k) c[0] += s.xyz[3 * f[k]] / 4.0, c[1] += s.xyz[3 * f[k] + 1] / 4.0;
            s.c2.insert(s.c2.end(), c, c + 2);
        }
    return s;
}

void surface(double x, double y, double lift, double* p) {
    p[0] = x, p[1] = y, p[2] = 0.02 * std::sin(3.0 * x) * std::cos(2.0 * y) + lift;
}

CsearchInput input(const Side& m, const Side& s, const int64_t* buck, double maxiDist) {
    return CsearchInput{m.xyz.data(), (int64_t)m.xyz.size() / 3, s.xyz.data(), (int64_t)s.xyz.size() / 3,
                        (int64_t)m.faces.size() / 4, m.faces.data(), m.c2.data(), (int64_t)s.faces.size() / 4,
                        s.faces.data(), s.c2.data(), buck, maxiDist};
}

int64_t host_count(const CsearchInput& in) {
    ddpca_ips_t h = nullptr;
    if (ddpca_contact_search(in.mast_xyz, in.mast_nnode, in.slav_xyz, in.slav_nnode, in.nm, in.mast_segm, in.mast_2d, in.ns,
                             in.slav_segm, in.slav_2d, in.buck, in.maxiDist, &h) != 0)
        return -1;
    const int64_t n = ddpca_ips_count(h);
    ddpca_ips_destroy(h);
    return n;
}

bool refused(const CsearchInput& in) {
    try {
        (void)csearch_plan(in);
    } catch (const ApiError& e) {
        return e.code == DDPCA_EINVAL;
    }
    return false;
}

}  // namespace

int main() {
    const int64_t buck4[2] = {4, 4}, buck12[2] = {12, 12};
    double ms[5];
    int64_t pairs[3];
    auto flat = [](double u, double v, double* p) { p[0] = u, p[1] = v, p[2] = 0.0; };
    const Side fm = grid(8, flat), fs = grid(8, flat);
    {
        ddpca_ips R;
        const CsearchInput in = input(fm, fs, buck4, 1.0e12);
        csearch_two_pass_host(in, true, R, ms, pairs);
        double sum = 0.0;
        for (int64_t q = 0; q < R.n; ++q) sum += R.w[q];
        expect(R.n == 1024 && R.n == host_count(in) && pairs[2] == R.n, "coincident: 1024 points, as the host search");
        expect(std::abs(sum - 1.0) <= 1e-12, "coincident: weights sum to the unit square");
        std::printf("{\"case\": \"coincident\", \"pairs\": %ld, \"kept\": %ld, \"points\": %ld}\n", (long)pairs[0], (long)pairs[1],
                    (long)pairs[2]);
    }
    const Side cm = grid(12, [](double u, double v, double* p) { surface(u, v, 0.0, p); });
    const Side cs = grid(15, [](double u, double v, double* p) {
        const double c = std::cos(0.3), s = std::sin(0.3), du = 0.6 * (u - 0.5), dv = 0.6 * (v - 0.5);
        surface(0.5 + c * du - s * dv, 0.5 + s * du + c * dv, 1.0e-4, p);
    });
    for (const int64_t* buck : {buck4, buck12})
        for (double maxiDist : {1.0e12, 1.3e-4}) {
            ddpca_ips R;
            const CsearchInput in = input(cm, cs, buck, maxiDist);
            csearch_two_pass_host(in, true, R, ms, pairs);
            expect(R.n == host_count(in) && R.n > 0, "curved: as many points as the host search");
            if (maxiDist > 1.0) expect(R.n == 8832, "curved: 8832 points");
            std::printf("{\"case\": \"curved\", \"buck\": %ld, \"maxiDist\": %g, \"pairs\": %ld, \"kept\": %ld, \"points\": %ld}\n",
                        (long)buck[0], maxiDist, (long)pairs[0], (long)pairs[1], (long)pairs[2]);
        }
    {   // the selection: node ids only, then the flags on one hex per face
        const int64_t nn[2] = {(int64_t)cm.xyz.size() / 3, (int64_t)cs.xyz.size() / 3};
        std::vector<int64_t> el[2];
        const Side* side[2] = {&cm, &cs};
        for (int s = 0; s < 2; ++s)
            for (size_t f = 0; f < side[s]->faces.size() / 4; ++f) {
                for (int k = 0; k < 4; ++k) el[s].push_back(side[s]->faces[4 * f + k]);
                for (int k = 0; k < 4; ++k) el[s].push_back(side[s]->faces[4 * f + k]);  // surface ids only: no second layer here
            }
        ddpca_ips R;
        csearch_two_pass_host(input(cm, cs, buck4, 1.3e-4), false, R, ms, pairs);
        std::vector<uint8_t> fm2(el[0].size() / 8), fs2(el[1].size() / 8), hm(fm2.size()), hs(fs2.size());
        const int any = refine_flags(R, nn[0], nn[1], (int64_t)fm2.size(), el[0].data(), (int64_t)fs2.size(), el[1].data(),
                                     fm2.data(), fs2.data());
        const int ref = ddpca_refine_select(cm.xyz.data(), nn[0], cs.xyz.data(), nn[1], (int64_t)cm.faces.size() / 4,
                                            cm.faces.data(), cm.c2.data(), (int64_t)cs.faces.size() / 4, cs.faces.data(),
                                            cs.c2.data(), buck4, 1.3e-4, (int64_t)hm.size(), el[0].data(), (int64_t)hs.size(),
                                            el[1].data(), hm.data(), hs.data());
        expect(any == ref && fm2 == hm && fs2 == hs, "refine selection equals the host's");
    }
    {   // no slave faces; the refusals
        Side none = cs;
        none.faces.clear(), none.c2.clear();
        ddpca_ips R;
        csearch_two_pass_host(input(cm, none, buck4, 1.0e12), true, R, ms, pairs);
        expect(R.n == 0 && pairs[0] == 0, "no slave faces: no points");
        Side bad = fm;
        bad.xyz[23] = std::nan("");
        expect(refused(input(bad, fs, buck4, 1.0e12)), "non-finite coordinate refused");
        bad = fm;
        bad.faces[21] = bad.faces[20];
        expect(refused(input(bad, fs, buck4, 1.0e12)), "coincident corners refused");
        bad = fm;
        for (int a = 0; a < 3; ++a) bad.xyz[3 * bad.faces[1] + a] = bad.xyz[3 * bad.faces[0] + a] + (a == 0 ? 2.0e-7 : 0.0);
        expect(refused(input(bad, fs, buck4, 1.0e12)), "trip cap above 2^20 refused");
    }
    std::printf("{\"ok\": %s, \"failures\": %d}\n", failures == 0 ? "true" : "false", failures);
    return failures == 0 ? 0 : 1;
}
