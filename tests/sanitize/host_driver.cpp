// Sanitizer driver for the host C++ of libddpca_amd (SURVEY §5 "race detection / sanitizers").
//
// Built by tests/sanitize/Makefile from the host translation units only (capi_builder, capi_host,
// capi_multigrid, csearch, errors, lagrange, admm_plan, mass_plan, mcontact, mgpis_plan, multigrid, multiscale, sparse, writers) with
// -fsanitize=address,undefined; no device objects, no GPU.  It drives the setup code that produces
// every GPU operand through the C ABI the tests use:
//   * the problem generators (BEAM single / DD, the two-block contact frictionless and Coulomb,
//     the synthetic DEHW chain) -> MCONTACT::ESTABLISH (mortar operators, MCONTACT.h:181-896),
//     MULTIGRID's uniform pipeline (MULTIGRID.h:756-1255), both coarse spaces (MULTISCALE and
//     MULTISCALE_1, MCONTACT.h:898-1536, 1680-1870), the rank-local builds of 2 and 4 ranks;
//     every array and operator the C ABI exposes is read and folded into a checksum;
//   * a general octree through ddpca_multigrid_* (REFINE with all seven patterns and spliFlag
//     chains, GRLE_CHECK, CURVEDS planSurf, TRANSFER with the hanging level, PATCH, STIF_MATR,
//     CONSTRAINT with nodal rotations), then as a problem subdomain;
//   * CSEARCH's contact search and ADAPTIVE_REFINE's selection on two facing surfaces;
//   * the result-file writers;
//   * the surface-mass batch's host setup (mass_plan.cpp, called directly): ELL-64 packing, pair
//     detection, spectrum bounds against a dense eigensolve, Chebyshev step counts;
//   * the host setup of an MGPIS device handle (mgpis_plan.cpp, called directly): the SELL-BSR3 level
//     plan of a two-member batch with and without coordinates, the value records of every storage
//     type, lattice and explicit transfers, a nine-parent node, the colour plan, the coarse packing;
//     on the octree above the block transfer entries and the band of the locally refined fine level;
//   * the host setup of the ADMM handle (admm_plan.cpp, called directly on the problems cast to
//     Problem*): the workspace layout and tables, every SELL-64 interface operator, the coupling and
//     hanging rows against products formed term by term from the Interface's operators (tolerance
//     (k - 1) eps sum |terms| per row), both branches of the fused decision, the coarse right-hand
//     side's slots of two-rank layouts against the one-rank plan bit for bit, the
//     DOUBLE_M_1 and LATIN DOUBLE_M hierarchies, the prolongation tables on the rotated octree, a rank
//     without subdomains, and the plan's refusals (an entry off the interface graph, baseReco off the
//     free dofs, a workspace index of 2^31);
//   * the refused-argument paths (bad indices, reversed pointers) of those entry points.
// The reference-comparison harnesses (oracle/ref_multigrid, ref_csearch, ref_refine,
// ref_lagrange_host) are linked to the same sanitized objects by the Makefile's `ref` target.
// Exit status 0 and no sanitizer report = clean.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <climits>
#include <cstring>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "admm_plan.hpp"
#include "common.hpp"
#include "ddpca_amd.h"
#include "mass_plan.hpp"
#include "mgpis_bytes.hpp"
#include "mgpis_plan.hpp"
#include "problem.hpp"
#include "subdomain_ops.hpp"

namespace ddpca {
MULTIGRID* multigrid_of(ddpca_multigrid_t h, bool* built);  // capi_multigrid.cpp
}

namespace {

int g_fail = 0;
void plan_general(const ddpca::MULTIGRID& g);  // the MGPIS plan on run_octree's tree, below
void admm_plan_octree(ddpca_multigrid_t g);     // the ADMM plan on it as a problem subdomain, below

void ok(int rc, const char* what) {
    if (rc < 0) {
        std::fprintf(stderr, "FAIL %s: %s\n", what, ddpca_last_error());
        ++g_fail;
    }
}

void refused(int rc, const char* what) {
    if (rc >= 0) {
        std::fprintf(stderr, "FAIL %s: accepted a bad argument\n", what);
        ++g_fail;
    }
}

double fold(const void* d, int64_t n, int dt) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        double v = 0.0;
        switch (dt) {
            case 0: v = static_cast<const double*>(d)[i]; break;
            case 1: v = (double)static_cast<const int64_t*>(d)[i]; break;
            case 2: v = (double)static_cast<const int32_t*>(d)[i]; break;
            default: v = (double)static_cast<const uint8_t*>(d)[i]; break;
        }
        s += std::isfinite(v) ? std::fabs(v) * (1.0 + (double)(i % 7)) : 0.0;
    }
    return s;
}

// reads one view; returns its checksum (0 when the view is refused, e.g. no coarse space)
double view(ddpca_problem_t p, const std::string& name, int64_t idx, int64_t lev, bool must = true) {
    const void* d = nullptr;
    int64_t n = 0;
    int dt = 0;
    const int rc = ddpca_problem_view(p, name.c_str(), idx, lev, &d, &n, &dt);
    if (rc < 0) {
        if (must) ok(rc, name.c_str());
        return 0.0;
    }
    return fold(d, n, dt);
}

double view_csr(ddpca_problem_t p, const std::string& base, int64_t idx, int64_t lev, bool must = true) {
    double s = 0.0;
    for (const char* part : {":shape", ":ptr", ":col", ":val"}) s += view(p, base + part, idx, lev, must);
    return s;
}

int64_t view_i64(ddpca_problem_t p, const char* name, int64_t idx, int64_t k) {
    const void* d = nullptr;
    int64_t n = 0;
    int dt = 0;
    ok(ddpca_problem_view(p, name, idx, 0, &d, &n, &dt), name);
    return (d && k < n && dt == 1) ? static_cast<const int64_t*>(d)[k] : 0;
}

// every array and operator of an established problem
double read_all(ddpca_problem_t p, int64_t muscSett, bool latin, const std::vector<uint8_t>& owned) {
    const int64_t nsub = view_i64(p, "sizes", 0, 0), nint = view_i64(p, "sizes", 0, 1);
    double s = 0.0;
    for (int64_t tv = 0; tv < nsub; ++tv) {
        for (const char* a : {"coords", "maxiLeve", "leveCount", "freeCount", "consFlag", "freeIndex", "consForc",
                              "dispForc", "exteForc", "consDofv"})
            s += view(p, a, tv, 0);
        const int64_t L = view_i64(p, "maxiLeve", tv, 0);
        for (int64_t l = 0; l <= L; ++l) {
            if (!owned[tv]) {  // another rank's subdomain: no operators here, refused
                const void* d = nullptr;
                int64_t n = 0;
                int dt = 0;
                refused(ddpca_problem_view(p, "K:ptr", tv, l, &d, &n, &dt), "view K of a subdomain not owned");
                continue;
            }
            s += view_csr(p, "K", tv, l);
            if (l < L) s += view_csr(p, "P", tv, l);
        }
        if (muscSett && owned[tv]) {
            s += view_csr(p, "accuProl", tv, 0);
            if (!latin) s += view_csr(p, "globTran_D_1", tv, 0);
        }
    }
    for (int64_t ts = 0; ts < nint; ++ts) {
        for (const char* a : {"iface_param", "iface_body", "inpoNgap", "pemaDiag", "ip_node", "ip_shap", "ip_basis",
                              "ip_gap", "ip_w"})
            s += view(p, a, ts, 0);
        for (int64_t side = 2 * ts; side < 2 * ts + 2; ++side) {
            s += view(p, "nodeCont", side, 0);
            for (const char* b : {"systMass", "systTran", "systTran_pena", "inteMass", "inteMass_pena", "inpoLagr",
                                  "inpoDisp", "inteInpo", "pemaInpo_r"})
                s += view_csr(p, b, side, 0);
            if (muscSett) {
                if (latin)
                    for (const char* b : {"globTran", "globTran_pena", "globTran_D"}) s += view_csr(p, b, side, 0, false);
                else
                    s += view_csr(p, "globTran_1", side, 0, false);
            }
        }
    }
    if (muscSett) {
        s += view(p, "baseReco", 0, 0) + view(p, "globForc_1", 0, 0) + view(p, "doleMcsc", 0, 0);
        s += view_csr(p, "globCoup_1", 0, 0);
    }
    // refused: out-of-range indices and unknown names
    const void* d = nullptr;
    int64_t n = 0;
    int dt = 0;
    refused(ddpca_problem_view(p, "consFlag", nsub, 0, &d, &n, &dt), "view subdomain nsub");
    refused(ddpca_problem_view(p, "consFlag", -1, 0, &d, &n, &dt), "view subdomain -1");
    refused(ddpca_problem_view(p, "ip_w", nint, 0, &d, &n, &dt), "view interface nint");
    refused(ddpca_problem_view(p, "systMass:ptr", 2 * nint, 0, &d, &n, &dt), "view side 2 nint");
    refused(ddpca_problem_view(p, "K:ptr", 0, 99, &d, &n, &dt), "view level 99");
    refused(ddpca_problem_view(p, "no_such_array", 0, 0, &d, &n, &dt), "view unknown name");
    return s;
}

struct Case {
    const char* kind;
    std::vector<double> params;
    int64_t musc;
    int ranks;  // 1: establish; > 1: establish_owned on every rank (contiguous blocks)
};

void run_case(const Case& c) {
    ddpca_problem_t probe = nullptr;
    ok(ddpca_problem_create(c.kind, c.params.data(), (int)c.params.size(), &probe), c.kind);
    if (!probe) return;
    const int64_t nsub = view_i64(probe, "sizes", 0, 0);
    ddpca_problem_destroy(probe);
    for (int r = 0; r < c.ranks; ++r) {
        ddpca_problem_t p = nullptr;
        ok(ddpca_problem_create(c.kind, c.params.data(), (int)c.params.size(), &p), c.kind);
        if (!p) return;
        std::vector<int64_t> dole(nsub, 1);
        if (c.musc) ok(ddpca_problem_set_coarse(p, c.musc, dole.data()), "set_coarse");
        std::vector<int32_t> owner(nsub);
        std::vector<uint8_t> owned(nsub, 1);
        for (int64_t tv = 0; tv < nsub; ++tv) {
            owner[tv] = (int32_t)(tv * c.ranks / nsub);
            owned[tv] = c.ranks == 1 || owner[tv] == r;
        }
        if (c.ranks == 1) ok(ddpca_problem_establish(p), "establish");
        else ok(ddpca_problem_establish_owned(p, owner.data(), r), "establish_owned");
        refused(ddpca_problem_set_coarse(p, 2, dole.data()), "set_coarse after establish");
        const double s = read_all(p, c.musc, c.musc == 1, owned);
        std::printf("{\"case\": \"%s\", \"params\": %zu, \"muscSett\": %ld, \"rank\": %d, \"ranks\": %d, \"checksum\": %.6e}\n",
                    c.kind, c.params.size(), (long)c.musc, r, c.ranks, s);
        ddpca_problem_destroy(p);
    }
}

// ---- a general octree: a 2 x 2 x 1 box refined with every pattern, curved top face
struct Tree {
    std::vector<double> xyz;
    std::vector<int64_t> corner, parent, level, patt, cptr{0}, child;
};

// the curved top face z = 1 + 0.01 (x^2 + y^2): box nodes and CURVEDS grid points coincide bitwise
double top(double x, double y) { return 1.0 + 0.01 * (x * x + y * y); }

Tree box(int nx, int ny, int nz) {
    Tree t;
    auto id = [&](int i, int j, int k) { return (int64_t)(i + (nx + 1) * (j + (ny + 1) * k)); };
    for (int k = 0; k <= nz; ++k)
        for (int j = 0; j <= ny; ++j)
            for (int i = 0; i <= nx; ++i) t.xyz.insert(t.xyz.end(), {(double)i, (double)j, k == nz ? top(i, j) : 0.5 * k});
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                t.corner.insert(t.corner.end(), {id(i, j, k), id(i + 1, j, k), id(i + 1, j + 1, k), id(i, j + 1, k),
                                                 id(i, j, k + 1), id(i + 1, j, k + 1), id(i + 1, j + 1, k + 1),
                                                 id(i, j + 1, k + 1)});
                t.parent.push_back(-1);
                t.level.push_back(0);
                t.patt.push_back(-1);
                t.cptr.push_back(0);
            }
    return t;
}

template <typename T>
std::vector<T> tree_get(ddpca_multigrid_t g, const char* what) {
    const void* d = nullptr;
    int64_t n = 0;
    int dt = 0;
    ok(ddpca_multigrid_tree(g, what, &d, &n, &dt), what);
    const T* p = static_cast<const T*>(d);
    return p ? std::vector<T>(p, p + n) : std::vector<T>();
}

void run_octree() {
    const int nx = 4, ny = 4, nz = 2;
    Tree t = box(nx, ny, nz);
    const int64_t nnode = (int64_t)t.xyz.size() / 3, nelem = (int64_t)t.parent.size();
    ddpca_multigrid_t g = nullptr;
    ok(ddpca_multigrid_create(nnode, t.xyz.data(), nelem, t.corner.data(), t.parent.data(), t.level.data(),
                              t.patt.data(), t.cptr.data(), nullptr, &g),
       "multigrid_create");
    if (!g) return;
    // round 1: every element 8-way, spliFlag on some children (a hanging level in round 2)
    std::vector<int64_t> elem, patt, fe, fc;
    for (int64_t e = 0; e < nelem; ++e) {  // (all seven patterns: ref_multigrid_san "refine")
        elem.push_back(e);
        patt.push_back(0);
    }
    fe = {0, 0, 7};
    fc = {1, 6, 0};
    // a curved top face: CURVEDS point grid over z = 1 + 0.05 (x^2 + y^2), planSurf of the new nodes
    const int64_t ni = 8 * nx + 1, nj = 8 * ny + 1;
    std::vector<double> surf;
    for (int64_t j = 0; j < nj; ++j)
        for (int64_t i = 0; i < ni; ++i) {
            const double x = nx * (double)i / (ni - 1), y = ny * (double)j / (nj - 1);
            surf.insert(surf.end(), {x, y, top(x, y)});
        }
    ddpca_curveds_t cs = nullptr;
    ok(ddpca_curveds_create(ni, nj, surf.data(), nullptr, &cs), "curveds_create");
    const int64_t *pptr = nullptr, *pnode = nullptr;
    const double* pxyz = nullptr;
    int64_t nplan = 0;
    if (cs) {
        const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tr[3] = {0, 0, 0};
        ok(ddpca_curveds_rigid(cs, R, tr), "curveds_rigid");
        ok(ddpca_curveds_plan(cs, g, (int64_t)elem.size(), elem.data(), &pptr, &pnode, &pxyz, &nplan), "curveds_plan");
    }
    std::vector<int64_t> pp(pptr ? pptr : nullptr, pptr ? pptr + nplan + 1 : nullptr);
    std::vector<int64_t> pn(pnode ? pnode : nullptr, pnode ? pnode + (nplan ? pp.back() : 0) : nullptr);
    std::vector<double> px(pxyz ? pxyz : nullptr, pxyz ? pxyz + 3 * nplan : nullptr);
    // refused first (the tree must stay as it was): reversed plan_ptr, spliFlag child 9
    if (nplan >= 2) {
        std::vector<int64_t> bad(pp);
        std::swap(bad[0], bad[1]);
        bad[0] = 0;
        bad[1] = pp[2] + 1;
        refused(ddpca_multigrid_refine(g, (int64_t)elem.size(), elem.data(), patt.data(), nplan, bad.data(), pn.data(),
                                       px.data(), 0, nullptr, nullptr),
                "refine reversed plan_ptr");
    }
    {
        const int64_t bfe = 0, bfc = 9;
        refused(ddpca_multigrid_refine(g, (int64_t)elem.size(), elem.data(), patt.data(), 0, nullptr, nullptr, nullptr, 1,
                                       &bfe, &bfc),
                "refine spliFlag child 9");
    }
    if ((int64_t)tree_get<int64_t>(g, "parent").size() != nelem) {
        std::fprintf(stderr, "FAIL refused refine changed the tree\n");
        ++g_fail;
    }
    ok(ddpca_multigrid_refine(g, (int64_t)elem.size(), elem.data(), patt.data(), nplan, pp.empty() ? nullptr : pp.data(),
                              pn.empty() ? nullptr : pn.data(), px.empty() ? nullptr : px.data(), (int64_t)fe.size(),
                              fe.data(), fc.data()),
       "refine round 1");
    // round 2: the children spliFlag selected, pattern 0 (GRLE_CHECK balances their neighbours)
    auto next = tree_get<int64_t>(g, "nextSplit");
    std::vector<int64_t> p0(next.size(), 0);
    if (!next.empty())
        ok(ddpca_multigrid_refine(g, (int64_t)next.size(), next.data(), p0.data(), 0, nullptr, nullptr, nullptr, 0,
                                  nullptr, nullptr),
           "refine round 2");
    if (cs) ddpca_curveds_destroy(cs);
    const auto coor = tree_get<double>(g, "nodeCoor");
    const size_t nel = tree_get<int64_t>(g, "parent").size();
    const int64_t nn = (int64_t)coor.size() / 3;
    // boundary data: x = 0 clamped, a load on x = nx, rotations on every 7th node, bad dofs refused
    std::vector<int64_t> cd, fi, rn;
    std::vector<double> cv, fv, rv;
    for (int64_t i = 0; i < nn; ++i) {
        if (coor[3 * i] == 0.0)
            for (int a = 0; a < 3; ++a) cd.push_back(3 * i + a), cv.push_back(0.0);
        if (coor[3 * i] == (double)nx) fi.push_back(3 * i + 2), fv.push_back(-1.0);
        if (i % 7 == 3 && coor[3 * i] > 0.0) {
            const double c = std::cos(0.3), s = std::sin(0.3);
            rn.push_back(i);
            rv.insert(rv.end(), {c, -s, 0, s, c, 0, 0, 0, 1});
        }
    }
    ok(ddpca_multigrid_set(g, "consDofv", (int64_t)cd.size(), cd.data(), cv.data()), "set consDofv");
    ok(ddpca_multigrid_set(g, "exteForc", (int64_t)fi.size(), fi.data(), fv.data()), "set exteForc");
    ok(ddpca_multigrid_set(g, "nodeRota", (int64_t)rn.size(), rn.data(), rv.data()), "set nodeRota");
    const double mat[2] = {2.1e11, 0.3};
    ok(ddpca_multigrid_set(g, "material", 2, nullptr, mat), "set material");
    for (int64_t bad : {(int64_t)-1, (int64_t)-2, 3 * nn}) {
        const double v = 1.0;
        refused(ddpca_multigrid_set(g, "consDofv", 1, &bad, &v), "set consDofv bad dof");
        refused(ddpca_multigrid_set(g, "exteForc", 1, &bad, &v), "set exteForc bad dof");
    }
    ok(ddpca_multigrid_build(g, nullptr), "multigrid_build");
    double s = 0.0;
    for (const char* w : {"posiNode", "nodeCoor", "leveCount", "freeCount", "consFlag", "consForc", "dispForc"}) {
        const void* d = nullptr;
        int64_t n = 0;
        int dt = 0;
        ok(ddpca_multigrid_view(g, w, 0, &d, &n, &dt), w);
        s += d ? fold(d, n, dt) : 0.0;
    }
    // as subdomain 0 of a one-subdomain problem (the builder's general-tree path)
    ddpca_problem_t p = nullptr;
    ok(ddpca_problem_empty(1, 0, &p), "problem_empty");
    if (p) {
        ok(ddpca_problem_set_subdomain_multigrid(p, 0, g), "set_subdomain_multigrid");
        refused(ddpca_problem_set_subdomain_multigrid(p, 1, g), "set_subdomain_multigrid tv 1");
        ok(ddpca_problem_finalize(p), "finalize");
        std::vector<uint8_t> owned{1};
        s += read_all(p, 0, false, owned);
        ddpca_problem_destroy(p);
    }
    std::printf("{\"case\": \"octree\", \"nodes\": %ld, \"elements\": %zu, \"planSurf\": %ld, \"checksum\": %.6e}\n", (long)nn, nel,
                (long)nplan, s);
    bool built = false;
    plan_general(*ddpca::multigrid_of(g, &built));
    admm_plan_octree(g);
    ddpca_multigrid_destroy(g);
}

// ---- CSEARCH on two facing, non-matching, slightly curved surfaces
void run_csearch() {
    // master: 6 x 6 quads on z = 0; slave: 9 x 9 quads on z = 1e-3 + small bump, offset in x/y
    auto grid = [](int n, double off, double z0, double bump, std::vector<double>& xyz, std::vector<int64_t>& segm,
                   std::vector<double>& uv) {
        for (int j = 0; j <= n; ++j)
            for (int i = 0; i <= n; ++i) {
                const double x = off + (double)i / n, y = off + (double)j / n;
                xyz.insert(xyz.end(), {x, y, z0 + bump * std::sin(3.0 * x) * std::sin(2.0 * y)});
            }
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) {
                const int64_t a = i + (n + 1) * j;
                segm.insert(segm.end(), {a, a + 1, a + n + 2, a + n + 1});
                uv.insert(uv.end(), {(double)i, (double)j, (double)i + 1, (double)j, (double)i + 1, (double)j + 1,
                                     (double)i, (double)j + 1});
            }
    };
    std::vector<double> mx, sx, mu, su;
    std::vector<int64_t> ms, ss;
    grid(6, 0.0, 0.0, 0.0, mx, ms, mu);
    grid(9, 0.05, 1.0e-3, 2.0e-4, sx, ss, su);
    const int64_t nm = (int64_t)ms.size() / 4, ns = (int64_t)ss.size() / 4;
    const int64_t buck[3] = {4, 4, 1};
    ddpca_ips_t ips = nullptr;
    ok(ddpca_contact_search(mx.data(), (int64_t)mx.size() / 3, sx.data(), (int64_t)sx.size() / 3, nm, ms.data(), mu.data(),
                            ns, ss.data(), su.data(), buck, 0.1, &ips),
       "contact_search");
    int64_t nip = 0;
    double s = 0.0;
    if (ips) {
        nip = ddpca_ips_count(ips);
        std::vector<int64_t> node(8 * nip);
        std::vector<double> shap(8 * nip), basis(9 * nip), gap(nip), w(nip);
        ok(ddpca_ips_get(ips, node.data(), shap.data(), basis.data(), gap.data(), w.data()), "ips_get");
        s = fold(node.data(), 8 * nip, 1) + fold(shap.data(), 8 * nip, 0) + fold(basis.data(), 9 * nip, 0) +
            fold(gap.data(), nip, 0) + fold(w.data(), nip, 0);
        ddpca_ips_destroy(ips);
    }
    // ADAPTIVE_REFINE's selection: the "elements" are the faces' nodes repeated as hexes
    std::vector<int64_t> me, se;
    for (int64_t f = 0; f < nm; ++f)
        for (int k = 0; k < 8; ++k) me.push_back(ms[4 * f + k % 4]);
    for (int64_t f = 0; f < ns; ++f)
        for (int k = 0; k < 8; ++k) se.push_back(ss[4 * f + k % 4]);
    std::vector<uint8_t> msp(nm), ssp(ns);
    const int sel = ddpca_refine_select(mx.data(), (int64_t)mx.size() / 3, sx.data(), (int64_t)sx.size() / 3, nm, ms.data(),
                                        mu.data(), ns, ss.data(), su.data(), buck, 0.05, nm, me.data(), ns, se.data(),
                                        msp.data(), ssp.data());
    ok(sel, "refine_select");
    std::printf("{\"case\": \"csearch\", \"ips\": %ld, \"selected\": %d, \"checksum\": %.6e}\n", (long)nip, sel, s);
}

void run_writers() {
    const char* dir = std::getenv("TMPDIR") ? std::getenv("TMPDIR") : "/tmp";
    const std::string a = std::string(dir) + "/san_resuDisp.txt", b = std::string(dir) + "/san_resuCont.txt",
                      c = std::string(dir) + "/san_resuMoni.txt";
    std::vector<double> disp(3 * 50), gamma(3 * 20), basis(9 * 20), rows(7 * 12);
    std::vector<int32_t> stat(20);
    for (size_t i = 0; i < disp.size(); ++i) disp[i] = std::sin((double)i);
    for (size_t i = 0; i < gamma.size(); ++i) gamma[i] = std::cos((double)i);
    for (size_t i = 0; i < basis.size(); ++i) basis[i] = (double)(i % 9 == 0 || i % 9 == 4 || i % 9 == 8);
    for (size_t i = 0; i < stat.size(); ++i) stat[i] = (int32_t)(i % 3);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = 1.0 / (1.0 + (double)i);
    const int64_t rn[2] = {3, 17};
    std::vector<double> rot(18, 0.0);
    for (int k = 0; k < 2; ++k) rot[9 * k] = rot[9 * k + 4] = rot[9 * k + 8] = 1.0;
    ok(ddpca_write_resuDisp(a.c_str(), disp.data(), 50, 2, rn, rot.data()), "write_resuDisp");
    ok(ddpca_write_resuCont(b.c_str(), 0.0, 20, gamma.data(), stat.data(), basis.data()), "write_resuCont f0");
    ok(ddpca_write_resuCont(b.c_str(), 0.3, 20, gamma.data(), stat.data(), basis.data()), "write_resuCont f3");
    ok(ddpca_write_resuMoni(c.c_str(), rows.data(), 12, 7), "write_resuMoni");
    std::printf("{\"case\": \"writers\"}\n");
}

// a surface-mass-like SPD system: the 9-point lattice mass matrix kron(T, T), T = tridiag(1, 4, 1) / 6,
// cut to n rows and scaled on both sides by a positive diagonal in [0.5, 2]
ddpca::Csr mass_like(int64_t n, double seed) {
    const int64_t m = (int64_t)std::ceil(std::sqrt((double)n));
    auto t = [](int64_t a, int64_t b) { return a == b ? 4.0 / 6.0 : 1.0 / 6.0; };
    auto d = [&](int64_t i) { return 1.25 + 0.75 * std::sin(seed + 1.7 * (double)i); };
    ddpca::Csr A;
    A.nrow = A.ncol = n;
    A.ptr.assign(1, 0);
    for (int64_t r = 0; r < n; ++r) {
        const int64_t i = r / m, j = r % m;
        for (int64_t i2 = std::max<int64_t>(i - 1, 0); i2 <= std::min(i + 1, m - 1); ++i2)
            for (int64_t j2 = std::max<int64_t>(j - 1, 0); j2 <= std::min(j + 1, m - 1); ++j2) {
                const int64_t c = i2 * m + j2;
                if (c >= n) continue;
                A.col.push_back((int32_t)c);
                A.val.push_back(d(r) * t(i, i2) * t(j, j2) * d(c));
            }
        A.ptr.push_back((int64_t)A.col.size());
    }
    return A;
}

// eigenvalue range of D^-1/2 M D^-1/2 (= that of D^-1 M) by cyclic Jacobi rotations, dense
void dense_spectrum(const ddpca::Csr& M, double* lmin, double* lmax) {
    const int64_t n = M.nrow;
    std::vector<double> S((size_t)n * n, 0.0), dg(n, 0.0);
    for (int64_t r = 0; r < n; ++r)
        for (int64_t k = M.ptr[r]; k < M.ptr[r + 1]; ++k)
            if (M.col[k] == r) dg[r] = M.val[k];
    for (int64_t r = 0; r < n; ++r)
        for (int64_t k = M.ptr[r]; k < M.ptr[r + 1]; ++k) S[r * n + M.col[k]] = M.val[k] / std::sqrt(dg[r] * dg[M.col[k]]);
    for (int sweep = 0; sweep < 30; ++sweep) {
        double offd = 0.0;
        for (int64_t p = 0; p < n; ++p)
            for (int64_t q = p + 1; q < n; ++q) offd += S[p * n + q] * S[p * n + q];
        if (offd < 1e-28) break;
        for (int64_t p = 0; p < n; ++p)
            for (int64_t q = p + 1; q < n; ++q) {
                if (S[p * n + q] == 0.0) continue;
                const double th = (S[q * n + q] - S[p * n + p]) / (2.0 * S[p * n + q]);
                const double tt = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
                const double c = 1.0 / std::sqrt(tt * tt + 1.0), s = tt * c;
                for (int64_t k = 0; k < n; ++k) {  // columns p, q, then rows p, q
                    const double a = S[k * n + p], b = S[k * n + q];
                    S[k * n + p] = c * a - s * b;
                    S[k * n + q] = s * a + c * b;
                }
                for (int64_t k = 0; k < n; ++k) {
                    const double a = S[p * n + k], b = S[q * n + k];
                    S[p * n + k] = c * a - s * b;
                    S[q * n + k] = s * a + c * b;
                }
            }
    }
    *lmin = *lmax = S[0];
    for (int64_t i = 0; i < n; ++i) *lmin = std::min(*lmin, S[i * n + i]), *lmax = std::max(*lmax, S[i * n + i]);
}

// MassBatch's host setup (mass_plan.cpp) on the paired batch [A0, A1, A0, A1] of 37 and 200 rows:
// one chunk and four, both with a ragged last chunk, 640 padded rows, R = 320
void run_mass_plan() {
    auto check = [](bool good, const char* what) {
        if (!good) {
            std::fprintf(stderr, "FAIL mass_plan: %s\n", what);
            ++g_fail;
        }
    };
    const ddpca::Csr A0 = mass_like(37, 0.3), A1 = mass_like(200, 1.1), B0 = A0, B1 = A1;
    const std::vector<const ddpca::Csr*> A = {&A0, &A1, &A0, &A1};
    const std::vector<int64_t> roff = {0, 64, 320, 384};
    const int64_t nrow = 640;
    const ddpca::MassPlan P = ddpca::mass_plan(A, roff, nrow, true);
    check(P.nch == 10 && P.paired && P.cheb, "10 chunks, paired, Chebyshev bounds");
    check(!ddpca::mass_plan({&A0, &A1, &B0, &B1}, roff, nrow, false).paired, "distinct copies do not pair");
    // the packed product against the CSR product, slot order = entry order: equal exactly
    std::vector<double> x(nrow), y(nrow, 0.0);
    for (int64_t i = 0; i < nrow; ++i) x[i] = std::sin(0.37 * (double)i) + 0.1 * std::cos(5.1 * (double)i);
    for (size_t s = 0; s < A.size(); ++s)
        for (int64_t r = 0; r < A[s]->nrow; ++r)
            for (int64_t k = A[s]->ptr[r]; k < A[s]->ptr[r + 1]; ++k) y[roff[s] + r] += A[s]->val[k] * x[roff[s] + A[s]->col[k]];
    bool same = true, dinv = true;
    for (int64_t g = 0; g < nrow; ++g) {
        const int64_t c = g / 64, lane = g % 64;
        double sum = 0.0;
        for (int64_t q = P.off[c]; q < P.off[c] + P.slots[c]; ++q) sum += P.val[q * 64 + lane] * x[P.col[q * 64 + lane]];
        same = same && sum == y[g];
    }
    for (size_t s = 0; s < A.size(); ++s)
        for (int64_t r = 0; r < A[s]->nrow; ++r)
            for (int64_t k = A[s]->ptr[r]; k < A[s]->ptr[r + 1]; ++k)
                if (A[s]->col[k] == r) dinv = dinv && P.dinv[roff[s] + r] == 1.0 / A[s]->val[k];
    check(same, "ELL product equals the CSR product");
    check(dinv, "D^-1");
    check(P.cb == std::vector<int64_t>({0, 1, 5, 6, 10}) && P.csys == std::vector<int32_t>({0, 1, 1, 1, 1, 2, 3, 3, 3, 3}),
          "chunk bounds and systems");
    // [lam_lo, lam_hi] brackets the spectrum of D^-1 M (the 37-row system, dense)
    double lmin = 0.0, lmax = 0.0;
    dense_spectrum(A0, &lmin, &lmax);
    check(P.lam_lo[0] > 0.0 && P.lam_lo[0] <= lmin && lmax <= P.lam_hi[0], "bounds bracket the 37-row spectrum");
    check(P.lam_lo[2] == P.lam_lo[0] && P.lam_hi[2] == P.lam_hi[0], "twins share their bounds");
    // step counts: K = ceil(ln(4 sqrt(kappa) / rtol) / ln sigma), sigma = (sqrt(kappa) + 1) / (sqrt(kappa) - 1)
    const double rtol = 1.0e-14;
    const ddpca::ChebPlan C = ddpca::cheb_plan(P.lam_lo, P.lam_hi, rtol);
    int64_t K = 0;
    bool steps = C.ks.size() == A.size();
    for (size_t s = 0; steps && s < A.size(); ++s) {
        const double sk = std::sqrt(P.lam_hi[s] / P.lam_lo[s]);
        const int64_t ks = std::max<int64_t>(1, (int64_t)std::ceil(std::log(4.0 * sk / rtol) / std::log((sk + 1.0) / (sk - 1.0))));
        steps = C.ks[s] == ks;
        K = std::max(K, ks);
    }
    check(steps && C.K == K, "Chebyshev step counts");
    check(K <= ddpca::kChebMax && C.coef.size() == (size_t)(2 * K) * A.size() && C.ith.size() == A.size(), "coefficients");
    check(ddpca::cheb_plan(P.lam_lo, P.lam_hi, 1.0e-300).coef.empty(), "no coefficients past kChebMax steps");
    std::printf("{\"case\": \"mass_plan\", \"lam\": [%.6f, %.6f], \"dense\": [%.6f, %.6f], \"steps\": %lld}\n", P.lam_lo[0],
                P.lam_hi[0], lmin, lmax, (long long)K);
}

// ---- MgpisDevice's host setup (mgpis_plan.cpp), called directly
using namespace ddpca;

void pcheck(bool good, const char* what) {
    if (!good) {
        std::fprintf(stderr, "FAIL mgpis_plan: %s\n", what);
        ++g_fail;
    }
}

// A symmetric operator with nonsymmetric blocks on nodes at integer positions xyz, reference
// numbering: every pair within one step per axis (and, `far`, the listed extra pairs) coupled by
// -(M_d + N_d), M_d = I + d d^T / 4 |d|^2 even in d, N_d = 0.05 [d]_x odd in d, so block (j, i) is
// the transpose of block (i, j); diagonal blocks 30 I plus a symmetric part that varies by node.
Bsr3 coupled_op(const std::vector<std::array<int, 3>>& xyz, const std::vector<std::pair<int, int>>& far = {}) {
    const int64_t n = (int64_t)xyz.size();
    Bsr3 A;
    A.nb = A.mb = n;
    A.ptr.assign(1, 0);
    auto coupled = [&](int64_t i, int64_t j) {
        for (const auto& f : far)
            if ((f.first == i && f.second == j) || (f.first == j && f.second == i)) return true;
        for (int a = 0; a < 3; ++a)
            if (std::abs(xyz[i][a] - xyz[j][a]) > 1) return false;
        return true;
    };
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t j = 0; j < n; ++j) {
            if (!coupled(i, j)) continue;
            double d[3], b[9];
            for (int a = 0; a < 3; ++a) d[a] = (double)(xyz[j][a] - xyz[i][a]);
            if (i == j) {
                for (int a = 0; a < 3; ++a)
                    for (int c = 0; c < 3; ++c) b[3 * a + c] = (a == c ? 30.0 : 0.0) + 0.3 * std::sin(1.0 + (double)i + a + c);
            } else {
                const double d2 = std::max(1.0, d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                const double N[9] = {0, -d[2], d[1], d[2], 0, -d[0], -d[1], d[0], 0};
                for (int a = 0; a < 3; ++a)
                    for (int c = 0; c < 3; ++c) b[3 * a + c] = -((a == c ? 1.0 : 0.0) + 0.25 * d[a] * d[c] / d2 + 0.05 * N[3 * a + c]) / d2;
            }
            A.col.push_back((int32_t)j);
            A.val.insert(A.val.end(), b, b + 9);
        }
        A.ptr.push_back((int64_t)A.col.size());
    }
    return A;
}

// an n0 x n1 x n2 lattice, and its nodes renumbered level-ordered: those at even positions first, in
// the coarse lattice's lexicographic order (the reference numbering of a once-refined box)
std::vector<std::array<int, 3>> lattice_xyz(int n0, int n1, int n2, bool level_ordered) {
    std::vector<std::array<int, 3>> even, odd;
    for (int z = 0; z < n2; ++z)
        for (int y = 0; y < n1; ++y)
            for (int x = 0; x < n0; ++x)
                (level_ordered && (x % 2 || y % 2 || z % 2) ? odd : even).push_back({x, y, z});
    even.insert(even.end(), odd.begin(), odd.end());
    return even;
}

std::vector<double> as_coords(const std::vector<std::array<int, 3>>& xyz) {
    std::vector<double> c;
    for (const auto& p : xyz) c.insert(c.end(), {(double)p[0], (double)p[1], (double)p[2]});
    return c;
}

// trilinear stencil from the nodes at even positions (the first nc of xyz, doubled coarse positions)
Stencil trilinear(const std::vector<std::array<int, 3>>& xyz, int64_t nc) {
    Stencil S;
    S.nf = (int64_t)xyz.size();
    S.nc = nc;
    S.ptr.assign(1, 0);
    for (const auto& f : xyz) {
        for (int64_t c = 0; c < nc; ++c) {
            double w = 1.0;
            for (int a = 0; a < 3; ++a) w *= xyz[c][a] == f[a] ? 1.0 : std::abs(xyz[c][a] - f[a]) == 1 ? 0.5 : 0.0;
            for (int a = 0; a < 3; ++a) w *= f[a] % 2 == 0 && xyz[c][a] != f[a] ? 0.0 : 1.0;
            if (w != 0.0) S.col.push_back((int32_t)c), S.w.push_back(w);
        }
        S.ptr.push_back((int64_t)S.col.size());
    }
    return S;
}

double half_value(uint16_t h) {  // IEEE half -> double
    const int e = (h >> 10) & 31, m = h & 1023;
    const double v = e ? std::ldexp(1024.0 + m, e - 25) : std::ldexp((double)m, -24);
    return h & 0x8000 ? -v : v;
}

// block (slot, lane) of V, decoded from the layout as the kernels read it
void decode(const BlockValues& V, int64_t slot, int64_t lane, double* out) {
    if (V.vt == kValQ8) {
        const uint8_t* s = V.v8.data() + slot * 768;
        auto byte = [&](int k) { return s[256 * (k / 4) + 4 * lane + k % 4]; };
        const uint32_t bits = (uint32_t)byte(9) << 8 | (uint32_t)byte(10) << 16 | (uint32_t)byte(11) << 24;
        float sc;
        std::memcpy(&sc, &bits, 4);
        for (int k = 0; k < 9; ++k) out[k] = (double)sc * (double)(int8_t)byte(k);
    } else if (V.vt == kValH16) {
        const uint16_t* s = V.v16.data() + slot * 640;
        auto half = [&](int k) { return s[128 * (k / 2) + 2 * lane + k % 2]; };
        for (int k = 0; k < 9; ++k) out[k] = std::ldexp(half_value(half(k)), (int)(int16_t)half(9));
    } else if (V.vt == kVal32) {
        for (int k = 0; k < 9; ++k) out[k] = (double)V.v32[slot * 576 + slot_elem<float>(k, lane)];
    } else {
        for (int k = 0; k < 9; ++k) out[k] = V.v64[slot * 576 + slot_elem<double>(k, lane)];
    }
}

// the dense matrix a level plan's SELL arrays hold (3 nn square; pad slots add their zeros)
std::vector<double> sell_dense(const LevelPlan& P) {
    const int64_t n = 3 * P.nn;
    std::vector<double> D(n * n, 0.0);
    for (int64_t g = 0; g < P.nn; ++g)
        for (int64_t q = P.off[g / 64]; q < P.off[g / 64 + 1]; ++q)
            for (int ij = 0; ij < 9; ++ij)
                D[(3 * g + ij / 3) * n + 3 * P.col[q * 64 + g % 64] + ij % 3] += P.val[(q * 9 + ij) * 64 + g % 64];
    return D;
}

void plan_levels_and_records() {
    // two members of 37 and 70 nodes on level 1 (8 and 12 on level 0), positions in a 5 x 4 x 4 box;
    // member 0's node 3 is clamped in y only, member 1's node 0 fully
    const auto box = lattice_xyz(5, 4, 4, false);
    const std::vector<std::array<int, 3>> x0(box.begin(), box.begin() + 37), x1(box.begin(), box.begin() + 70);
    const Bsr3 K0 = coupled_op(x0), K1 = coupled_op(x1);
    const Bsr3 C0 = coupled_op({x0.begin(), x0.begin() + 8}), C1 = coupled_op({x1.begin(), x1.begin() + 12});
    const std::vector<double> c0 = as_coords(x0), c1 = as_coords(x1);
    std::vector<uint8_t> f0(3 * 37, 1), f1(3 * 70, 1);
    f0[3 * 3 + 1] = 0;
    f1[0] = f1[1] = f1[2] = 0;
    for (int with_coords = 0; with_coords < 2; ++with_coords) {
        std::vector<SubdomainOps> subs(2);
        subs[0].nnodes = {8, 37};
        subs[1].nnodes = {12, 70};
        subs[0].K = {&C0, &K0};
        subs[1].K = {&C1, &K1};
        subs[0].dof_free = f0.data();
        subs[1].dof_free = f1.data();
        if (with_coords) subs[0].coords = c0.data(), subs[1].coords = c1.data();
        const MgpisNumbering num = mgpis_numbering(subs, 0);
        const MgpisTuning tune;
        const LevelPlan P = plan_level(subs, num, 1, true, 0, tune);
        pcheck(P.nn == 192 && P.nch == 3 && P.noff == std::vector<int64_t>({0, 64}) && P.csub == std::vector<int32_t>({0, 1, 1}),
               "37 + 70 nodes pad to 64 + 128, the second member spans two chunks");
        // the masked operator, restated: identity on constrained dofs
        const int64_t n = 3 * P.nn;
        std::vector<double> E(n * n, 0.0);
        bool pads = true, inv = true;
        for (int s = 0; s < 2; ++s) {
            const Bsr3& A = *subs[s].K[1];
            const uint8_t* fr = subs[s].dof_free;
            const auto& p = num.perm[1][s];
            for (int64_t r = 0; r < A.nb; ++r)
                for (int64_t k = A.ptr[r]; k < A.ptr[r + 1]; ++k)
                    for (int ij = 0; ij < 9; ++ij) {
                        const int64_t j = A.col[k], a = ij / 3, b = ij % 3;
                        const bool fr_ab = fr[3 * r + a] && fr[3 * j + b];
                        E[(3 * (P.noff[s] + p[r]) + a) * n + 3 * (P.noff[s] + p[j]) + b] =
                            fr_ab ? A.val[9 * k + ij] : (j == r && a == b ? 1.0 : 0.0);
                    }
            // slots past a row's blocks and pad rows: a self column (their values are zero by the dense equality)
            for (int64_t g = P.noff[s]; g < P.noff[s] + pad64(P.nloc[s]); ++g) {
                int64_t others = 0, want = 0;
                for (int64_t q = P.off[g / 64]; q < P.off[g / 64 + 1]; ++q) others += P.col[q * 64 + g % 64] != g;
                for (int64_t r = 0; r < A.nb; ++r)
                    if (P.noff[s] + p[r] == g) want = A.ptr[r + 1] - A.ptr[r] - 1;
                pads = pads && others == want;
            }
            // minv x the padded diagonal block: identity on free dofs, zero elsewhere
            for (int64_t r = 0; r < A.nb; ++r) {
                const int64_t g = P.noff[s] + p[r];
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) {
                        double sum = 0.0;
                        for (int c = 0; c < 3; ++c) sum += P.minv[9 * g + 3 * a + c] * E[(3 * g + c) * n + 3 * g + b];
                        const bool fr_ab = fr[3 * r + a] && fr[3 * r + b];
                        inv = inv && (fr_ab ? std::fabs(sum - (a == b)) <= 1e-12 : P.minv[9 * g + 3 * a + b] == 0.0);
                    }
            }
        }
        pcheck(sell_dense(P) == E, "decoding the SELL gives the masked operator exactly");
        pcheck(pads, "pad slots and pad rows carry a self column");
        pcheck(inv, "minv times the diagonal block is the identity on free dofs, zero elsewhere");
        bool c16 = P.col16.size() == P.col.size(), sym = true;
        for (size_t i = 0; c16 && i < P.col.size(); ++i) {
            const int64_t q = (int64_t)i / 64, c = std::upper_bound(P.off.begin(), P.off.end(), q) - P.off.begin() - 1;
            c16 = P.col16[i] == P.col[i] - (c * 64 + (int64_t)i % 64);
        }
        pcheck(c16, "col16 is col minus the row index");
        const std::vector<float> m32 = smoother_inverse_fp32(P.minv, true, true);
        for (int64_t g = 0; g < P.nn; ++g)
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) sym = sym && m32[9 * g + 3 * a + b] == m32[9 * g + 3 * b + a];
        pcheck(sym, "minv32 is exactly symmetric");
        // records: each storage type within its bound of val; fp64 exact
        for (int vt : {kVal64, kVal32, kValH16, kValQ8}) {
            const BlockValues V = pack_values(P, vt);
            bool bound = V.ok;
            for (int64_t q = 0; q < P.nslots; ++q)
                for (int64_t lane = 0; lane < 64; ++lane) {
                    double v[9], d[9], m = 0.0;
                    for (int k = 0; k < 9; ++k) v[k] = P.val[(q * 9 + k) * 64 + lane], m = std::max(m, std::fabs(v[k]));
                    decode(V, q, lane, d);
                    for (int k = 0; k < 9; ++k) {
                        const double e = std::fabs(d[k] - v[k]);
                        bound = bound && (vt == kVal64 ? e == 0.0 : vt == kVal32 ? e <= std::ldexp(std::fabs(v[k]), -24)
                                                          : vt == kValH16 ? e <= std::ldexp(m, -11) : e <= 0.5 * m / 127.0);
                    }
                }
            pcheck(bound, "a value copy lies within its format's bound of val");
        }
        // the record of block (i, j) is the transpose of the record of block (j, i): compare the
        // stored halves / bytes, exponent and scale included
        for (int vt : {kValH16, kValQ8}) {
            const BlockValues V = pack_values(P, vt);
            const int nv = vt == kValQ8 ? 12 : 10;
            auto rec = [&](int64_t q, int64_t lane, int k) -> int {
                return vt == kValQ8 ? V.v8[q * 768 + 256 * (k / 4) + 4 * lane + k % 4] : V.v16[q * 640 + 128 * (k / 2) + 2 * lane + k % 2];
            };
            bool tr = true;
            int64_t pairs = 0;
            for (int64_t g = 64; g < 64 + 70; ++g)  // member 1's rows that couple only free nodes
                for (int64_t q = P.off[g / 64]; q < P.off[g / 64 + 1]; ++q) {
                    const int64_t j = P.col[q * 64 + g % 64];
                    if (j == g || !(P.mask[g] == 7 && P.mask[j] == 7)) continue;
                    for (int64_t q2 = P.off[j / 64]; q2 < P.off[j / 64 + 1]; ++q2) {
                        if (P.col[q2 * 64 + j % 64] != g) continue;
                        ++pairs;
                        for (int k = 0; k < nv; ++k) tr = tr && rec(q, g % 64, k) == rec(q2, j % 64, k < 9 ? 3 * (k % 3) + k / 3 : k);
                    }
                }
            pcheck(tr && pairs > 100, "the record of block (i, j) is the transpose of that of block (j, i)");
        }
        // coarse: member 0's level-1 operator as a dense coarse matrix
        if (!with_coords) {
            std::vector<double> D = coarse_dense(subs[0], 1, num.perm[1][0], false), packed;
            const int64_t ld = coarse_pack(D, subs[0], 1, num.perm[1][0], 64, packed);
            bool zero = true;
            for (int64_t e = 0; e < 111; ++e) zero = zero && packed[(3 * 3 + 1) * ld + e] == 0.0 && packed[e * ld + 3 * 3 + 1] == 0.0;
            pcheck(ld == 112 && packed.size() == (size_t)(111 * 112) && zero && packed[0] == K0.val[0],
                   "packed coarse rows: stride a multiple of 4, constrained rows and columns zero");
            bool thrown = false;
            try {
                coarse_pack(D, subs[0], 1, num.perm[1][0], 37, packed);  // 112 > 3 * 37
            } catch (const ApiError& e) {
                thrown = e.code == DDPCA_ESTATE;
            }
            pcheck(thrown, "coarse row padding beyond the member is refused");
        }
    }
    // a block past the int8 record's range: no int8 copy, the level falls back to block-exponent fp16.
    // Entries of 1e39 are beyond fp32's largest number, which the packing refuses; at 1e41 the scale
    // max / 127 itself is no fp32 number any more
    for (double huge : {1e41, 1e39}) {
        Bsr3 B = coupled_op(x0);
        for (int k = 0; k < 9; ++k) B.val[9 * B.ptr[5] + k] = huge;
        std::vector<SubdomainOps> subs(1);
        subs[0].nnodes = {37};
        subs[0].K = {&B};
        std::vector<uint8_t> fr(3 * 37, 1);
        subs[0].dof_free = fr.data();
        const MgpisNumbering num = mgpis_numbering(subs, 0);
        const MgpisTuning tune;
        const LevelPlan P = plan_level(subs, num, 0, true, 0, tune);
        const BlockValues V8 = pack_values(P, kValQ8);
        const int fell_to = level_copy(P, kValQ8, 0, tune).vt;
        std::printf("{\"case\": \"mgpis_plan_int8_range\", \"entries\": %g, \"int8_ok\": %d, \"level_copy\": %d}\n", huge, (int)V8.ok, fell_to);
        const std::string at = "entries of " + std::to_string((int)std::log10(huge)) + " decades: ";
        pcheck(!V8.ok, (at + "int8 packing reports a scale out of range").c_str());
        pcheck(level_copy_type(3, 2, 3, tune) == kValQ8 && fell_to == kValH16, (at + "the level falls back to fp16").c_str());
        MgpisTuning t1;
        t1.h16_levels = 1;
        t1.q8_levels = 0;
        t1.col16 = false;
        pcheck(!P.col16.empty() && plan_level(subs, num, 0, true, 0, t1).col16.empty(), "the tuning switches col16 off");
        pcheck(level_copy_type(3, 1, 3, t1) == kVal32 && level_copy_type(3, 2, 3, t1) == kValH16 && level_copy_type(1, 2, 3, tune) == kVal32,
               "copy types follow the tuning's level counts");
    }
    // a chain of 33,000 nodes with one block coupling nodes 0 and 32,900: no 16-bit columns
    {
        Bsr3 A;
        A.nb = A.mb = 33000;
        A.ptr.assign(1, 0);
        const double I[9] = {4, 0, 0, 0, 4, 0, 0, 0, 4}, O[9] = {-1, 0, 0, 0, -1, 0, 0, 0, -1};
        for (int64_t i = 0; i < 33000; ++i) {
            std::vector<int64_t> cols = {i};
            if (i > 0) cols.push_back(i - 1);
            if (i + 1 < 33000) cols.push_back(i + 1);
            if (i == 0) cols.push_back(32900);
            if (i == 32900) cols.push_back(0);
            std::sort(cols.begin(), cols.end());
            for (int64_t j : cols) A.col.push_back((int32_t)j), A.val.insert(A.val.end(), j == i ? I : O, (j == i ? I : O) + 9);
            A.ptr.push_back((int64_t)A.col.size());
        }
        std::vector<SubdomainOps> subs(1);
        subs[0].nnodes = {33000};
        subs[0].K = {&A};
        std::vector<uint8_t> fr(3 * 33000, 1);
        subs[0].dof_free = fr.data();
        const MgpisNumbering num = mgpis_numbering(subs, 0);
        const LevelPlan P = plan_level(subs, num, 0, false, 0, MgpisTuning());
        pcheck(P.col16.empty() && P.minv.size() == (size_t)(3 * P.nn), "an offset of 32,900 leaves no col16");
    }
    // clev: the 256 MB / 12,288-row rule and the option
    {
        auto clev = [](std::vector<std::vector<int64_t>> nn, int opt) {
            std::vector<SubdomainOps> subs(nn.size());
            for (size_t s = 0; s < nn.size(); ++s) subs[s].nnodes = nn[s];
            int64_t n0 = 0;
            const int c = choose_coarse_level(subs, opt, &n0);
            return std::make_pair(c, n0);
        };
        const std::vector<int64_t> a = {10, 1000, 1500, 100000}, b = {10, 3000, 5000, 100000};
        pcheck(clev({a}, -1) == std::make_pair(2, (int64_t)4500), "one member: 162 MB on level 2 fits");
        pcheck(clev({a, a}, -1).first == 1, "two members: 324 MB do not, 144 MB on level 1 do");
        pcheck(clev({b}, -1).first == 0, "15,000 rows are too many, 648 MB too much");
        pcheck(clev({a}, 1).first == 1 && clev({a}, 9).first == 2 && clev({{50}}, -1) == std::make_pair(0, (int64_t)150),
               "the option, capped below the fine level; one level");
    }
}

// P of a transfer plan's explicit lists, dense (fine device node x coarse device node), and R
// from its child SELL
void lists_dense(const TransferPlan& T, const LevelShape& F, const LevelShape& C, std::vector<double>& P, std::vector<double>& R) {
    P.assign(F.nn * C.nn, 0.0);
    R.assign(C.nn * F.nn, 0.0);
    for (int64_t gf = 0; gf < F.nn; ++gf)
        for (int k = 0; k < 8 && T.ppar[k * F.nn + gf] >= 0; ++k) P[gf * C.nn + T.ppar[k * F.nn + gf]] += T.pw[k * F.nn + gf];
    for (int64_t j = 0; j < C.nn; ++j)
        for (int64_t q = T.roff[j / 64]; q < T.roff[j / 64 + 1]; ++q) R[j * F.nn + T.rcol[q * 64 + j % 64]] += T.rwt[q * 64 + j % 64];
}

void plan_transfers_and_colours() {
    // 3 x 3 x 3 -> 5 x 5 x 5, trilinear, the fine nodes level-ordered
    const auto xf = lattice_xyz(5, 5, 5, true);
    const Bsr3 Kf = coupled_op(xf), Kc = coupled_op({xf.begin(), xf.begin() + 27});
    Stencil S = trilinear(xf, 27);
    const std::vector<double> coords = as_coords(xf);
    std::vector<uint8_t> fr(3 * 125, 1);
    std::vector<SubdomainOps> subs(1);
    subs[0].nnodes = {27, 125};
    subs[0].K = {&Kc, &Kf};
    subs[0].S = {&S};
    subs[0].dof_free = fr.data();
    subs[0].coords = coords.data();
    const MgpisNumbering num = mgpis_numbering(subs, 0);
    MgpisTuning tune;
    const LevelPlan PC = plan_level(subs, num, 0, true, 0, tune), PF = plan_level(subs, num, 1, true, 0, tune);
    const TransferPlan TL = plan_transfer(subs, num, 1, PF, PC, tune);
    tune.lattice = false;
    const TransferPlan TX = plan_transfer(subs, num, 1, PF, PC, tune);
    tune.lattice = true;
    pcheck(TL.lat && TL.uw && TL.nrot == 0, "the trilinear lattice is taken as a lattice");
    pcheck(!TX.lat && TX.uw && TX.ppar == TL.ppar && TX.rcol == TL.rcol, "lattice flag off: explicit lists, uniform averaging");
    std::vector<double> P, R, E(PF.nn * PC.nn, 0.0);
    lists_dense(TX, PF, PC, P, R);
    for (int64_t i = 0; i < 125; ++i)
        for (int64_t e = S.ptr[i]; e < S.ptr[i + 1]; ++e) E[num.perm[1][0][i] * PC.nn + num.perm[0][0][S.col[e]]] = S.w[e];
    bool rt = true, codes = true;
    for (int64_t gf = 0; gf < PF.nn; ++gf)
        for (int64_t j = 0; j < PC.nn; ++j) rt = rt && R[j * PF.nn + gf] == P[gf * PC.nn + j];
    pcheck(P == E, "the lists applied as P reproduce the stencil exactly");
    pcheck(rt, "the child SELL applied as R is P^T exactly");
    // the lattice codes expand to the same parents and children
    for (int64_t gf = 0; gf < 125 && TL.lat; ++gf) {
        const uint32_t code = TL.ppk[gf] >> 29, p0 = TL.ppk[gf] & 0x1FFFFFFFu;
        std::vector<double> row(PC.nn, 0.0);
        const int np = 1 << __builtin_popcount(code);
        for (uint32_t q = 0; q < 8; ++q)
            if ((q & ~code) == 0) row[p0 + ((q & 1) ? TL.pstr[0] : 0) + ((q & 2) ? TL.pstr[1] : 0) + ((q & 4) ? TL.pstr[2] : 0)] += 1.0 / np;
        codes = codes && std::equal(row.begin(), row.end(), E.begin() + gf * PC.nn);
    }
    for (int64_t j = 0; j < 27 && TL.lat; ++j) {
        std::vector<double> row(PF.nn, 0.0);
        for (int q = 0; q < 27; ++q)
            if ((TL.rmsk[j] >> q) & 1u) {
                const int d[3] = {q % 3 - 1, (q / 3) % 3 - 1, q / 9 - 1};
                row[TL.rf0[j] + d[0] * TL.rstr[0] + d[1] * TL.rstr[1] + d[2] * TL.rstr[2]] += 1.0 / (1 << ((d[0] != 0) + (d[1] != 0) + (d[2] != 0)));
            }
        codes = codes && std::equal(row.begin(), row.end(), R.begin() + j * PF.nn);
    }
    pcheck(codes, "the lattice codes expand to the lists' parents and children");
    // not the identity on a coarse node: DDPCA_EINVAL
    {
        Stencil B = S;
        B.w[B.ptr[4]] = 0.5;
        subs[0].S = {&B};
        bool thrown = false;
        try {
            plan_transfer(subs, num, 1, PF, PC, tune);
        } catch (const ApiError& e) {
            thrown = e.code == DDPCA_EINVAL && std::string(e.what()) == "stencil is not identity on coarse nodes";
        }
        pcheck(thrown, "a stencil that is not the identity on a coarse node is refused");
        subs[0].S = {&S};
    }
    // a node with nine parents: the ninth goes to the block CSRs as w I
    {
        Stencil N;
        N.nf = 11;
        N.nc = 10;
        N.ptr.assign(1, 0);
        for (int i = 0; i < 10; ++i) N.col.push_back(i), N.w.push_back(1.0), N.ptr.push_back(i + 1);
        for (int c = 0; c < 9; ++c) N.col.push_back(c), N.w.push_back(1.0 / 9.0);
        N.ptr.push_back(19);
        LevelShape F, C;
        F.nn = C.nn = 64;
        F.nch = C.nch = 1;
        F.noff = C.noff = {0};
        F.nloc = {11};
        C.nloc = {10};
        std::vector<SubdomainOps> one(1);
        one[0].nnodes = {10, 11};
        one[0].S = {&N};
        MgpisNumbering id;
        id.perm = {{identity_order(10)}, {identity_order(11)}};
        const TransferPlan T = plan_transfer(one, id, 1, F, C, tune);
        const double w = 1.0 / 9.0;
        pcheck(!T.uw && !T.lat && T.nrot == 1 && T.nrotc == 1 && T.rot_row == std::vector<int32_t>({10}) &&
                   T.rot_par == std::vector<int32_t>({8}) && T.rotc_row == std::vector<int32_t>({8}) &&
                   T.rotc_kid == std::vector<int32_t>({10}) && T.rot_blk == std::vector<double>({w, 0, 0, 0, w, 0, 0, 0, w}) &&
                   T.ppar[7 * 64 + 10] == 7 && T.tent_sub[0] == 19,
               "the ninth parent runs as a w I block");
    }
    // colours on the 5 x 5 x 5 27-point operator
    const std::vector<float> m32 = smoother_inverse_fp32(PF.minv, true, true);
    const ColourPlan G = plan_colours(PF, kValH16, &m32, nullptr, tune);
    std::vector<int> colour(PF.nn, -1), seen(PF.nn, 0), chunk_colour(G.nchunk, -1);
    for (int k = 0; k < G.ncol; ++k)
        for (int64_t i = G.first[k]; i < G.first[k] + G.count[k]; ++i) chunk_colour[G.list[i]] = k;
    bool pad = true, split = true, proper = true;
    for (int64_t c = 0; c < G.nchunk; ++c)
        for (int64_t lane = 0; lane < 64; ++lane) {
            const int32_t r = G.rowidx[c * 64 + lane];
            if (r >= 0) colour[r] = chunk_colour[c], ++seen[r];
            else pad = pad && r == ~G.rowidx[c * 64];
        }
    for (int64_t g = 0; g < 125; ++g) pad = pad && seen[g] == 1;
    for (int64_t c = 0; c < G.nchunk; ++c)
        for (int64_t lane = 0; lane < 64; ++lane) {
            const int32_t g = G.rowidx[c * 64 + lane];
            if (g < 0) continue;
            std::vector<int64_t> row, lu;
            for (int64_t q = PF.off[g / 64]; q < PF.off[g / 64 + 1]; ++q)
                if (PF.col[q * 64 + g % 64] != g) row.push_back(PF.col[q * 64 + g % 64]);
            for (int64_t q = G.offl[c]; q < G.offl[c] + G.nsl[c] + G.nsu[c]; ++q) {
                const int64_t j = g + G.col16[q * 64 + lane];
                if (j == g) continue;  // a pad slot
                lu.push_back(j);
                split = split && (colour[j] < colour[g]) == (q < G.offu[c]);
                proper = proper && colour[j] != colour[g];
            }
            std::sort(row.begin(), row.end());
            std::sort(lu.begin(), lu.end());
            split = split && row == lu;
        }
    pcheck(G.ncol == 8 && proper, "8 colours, no two coupled rows share one");
    pcheck(pad, "every real row once in rowidx, pad lanes the complement of the chunk's first row");
    pcheck(split, "L + U + diagonal is the row, L exactly the columns of earlier colours");
    pcheck(G.launch_bytes.size() == (size_t)(2 * G.ncol + 1) && G.minvc.size() == (size_t)G.nchunk * 576 && !G.band,
           "launch_bytes has 2 K + 1 entries");
    ColourShape M = G;
    colour_byte_model(M, 4, true, true);
    pcheck(M.launch_bytes.size() == (size_t)(4 * G.ncol + 1), "colour SSOR's model has 4 K + 1 launches");
    std::printf("{\"case\": \"mgpis_plan\", \"colours\": %d, \"colour_chunks\": %lld, \"lattice\": %d}\n", G.ncol,
                (long long)G.nchunk, (int)TL.lat);
}

// the refined octree: block transfer entries (rotated nodes) and the locally refined fine level's band
void plan_general(const MULTIGRID& g) {
    const std::vector<SubdomainOps> subs = {subdomain_ops(g)};
    const int nlev = (int)subs[0].nnodes.size();
    const MgpisNumbering num = mgpis_numbering(subs, 0);
    MgpisTuning tune;
    std::vector<LevelPlan> P;
    for (int l = 0; l < nlev; ++l) P.push_back(plan_level(subs, num, l, true, 0, tune));
    int64_t blocks = 0;
    for (int l = 1; l < nlev; ++l) {
        const TransferPlan T = plan_transfer(subs, num, l, P[l], P[l - 1], tune);
        if (subs[0].S[l - 1]->bent.empty()) continue;
        using Ent = std::tuple<int32_t, int32_t, std::array<double, 9>>;
        std::vector<Ent> by_f, by_c;
        auto collect = [](const std::vector<int32_t>& row, const std::vector<int64_t>& ptr, const std::vector<int32_t>& other,
                          const std::vector<double>& blk, bool fine_rows, std::vector<Ent>& out) {
            for (size_t r = 0; r < row.size(); ++r)
                for (int64_t e = ptr[r]; e < ptr[r + 1]; ++e) {
                    std::array<double, 9> b;
                    std::copy(blk.begin() + 9 * e, blk.begin() + 9 * e + 9, b.begin());
                    out.push_back(fine_rows ? Ent{row[r], other[e], b} : Ent{other[e], row[r], b});
                }
            std::sort(out.begin(), out.end());
        };
        collect(T.rot_row, T.rot_ptr, T.rot_par, T.rot_blk, true, by_f);
        collect(T.rotc_row, T.rotc_ptr, T.rotc_kid, T.rotc_blk, false, by_c);
        blocks += (int64_t)by_f.size();
        pcheck(!T.uw && !T.lat && by_f == by_c && by_f.size() >= subs[0].S[l - 1]->bent.size(),
               "block entries: no uniform averaging, the same entry set by fine and by coarse node");
    }
    pcheck(blocks > 0, "the rotated octree has block transfer entries");
    const int L = nlev - 1;
    const std::vector<uint8_t> band = colour_band(subs, num, L, P[L], tune);
    int64_t nband = 0;
    for (uint8_t f : band) nband += f != 0;
    pcheck(!band.empty() && 5 * nband <= 3 * P[L].nloc[0], "the refined corner's band is under 60 % of the rows");
    if (!band.empty()) {
        const ColourPlan G = plan_colours(P[L], kVal32, nullptr, &band, tune);
        pcheck(G.band && (int)G.first.size() == G.ncol + 2 && G.count[G.ncol] > 0 && G.count[G.ncol + 1] > 0 &&
                   G.band_rows_sub[0] == nband && G.ring_rows_sub[0] > 0 && G.far_rows_sub[0] > 0 &&
                   nband + G.ring_rows_sub[0] + G.far_rows_sub[0] == P[L].nloc[0],
               "band mode: the colours cover the band, ring and far groups the rest");
    }
    tune.gs_band = false;
    pcheck(colour_band(subs, num, L, P[L], tune).empty(), "band flag off: no band");
    const ColourPlan A = plan_colours(P[L], kVal32, nullptr, nullptr, tune);
    double rows = 0.0;
    for (double r : A.rows_k) rows += r;
    pcheck(!A.band && (int)A.first.size() == A.ncol && rows == (double)P[L].nloc[0], "band flag off: the colours sweep every row");
    std::printf("{\"case\": \"mgpis_plan_general\", \"levels\": %d, \"fine_rows\": %lld, \"band\": %lld, \"block_entries\": %lld}\n",
                nlev, (long long)P[L].nloc[0], (long long)nband, (long long)blocks);
}

// ---- the byte model of the solve path (mgpis_bytes.cpp) on shapes small enough to tally by hand
MgpisBytes::Level bytes_level(std::vector<int64_t> nloc, std::vector<int64_t> nnzb, std::vector<int64_t> tent) {
    MgpisBytes::Level L;
    L.tblk_sub.assign(nloc.size(), 0);
    L.nloc = std::move(nloc);
    L.nnzb_sub = std::move(nnzb);
    L.tent_sub = std::move(tent);
    return L;
}

// vcycle_bytes of member s = {fine, below}, iteration_launches = launches (all three literals of the
// caller's tally), and the identities that tie the other figures to them
void bytes_check(const MgpisBytes& M, int s, double fine, double below, int64_t launches, const char* what) {
    double v[2], it[2], su[2];
    vcycle_bytes(M, s, v);
    iteration_bytes(M, s, it);
    setup_bytes(M, s, su);
    const int64_t nl = iteration_launches(M);
    if (v[0] != fine || v[1] != below || nl != launches) {
        std::fprintf(stderr, "FAIL mgpis_bytes: %s member %d: {%.17g, %.17g} and %lld launches, tallied {%.17g, %.17g} and %lld\n",
                     what, s, v[0], v[1], (long long)nl, fine, below, (long long)launches);
        ++g_fail;
    }
    const double n = (double)M.lev.back().nloc[s], nch = (double)((M.lev.back().nloc[s] + 63) / 64);
    const bool tied = it[0] == v[0] + fine_kernel_bytes(M, s) + 144.0 * n && it[1] == v[1] + 24.0 * nch &&
                      su[0] - v[0] == 120.0 * n && su[1] - v[1] == 16.0 * nch &&
                      fine_kernel_bytes(M, s) == fine_matrix_bytes(M, s, kVal64) + 120.0 * n;
    if (!tied) {
        std::fprintf(stderr, "FAIL mgpis_bytes: %s member %d: iteration / setup bytes off the V-cycle's\n", what, s);
        ++g_fail;
    }
}

void byte_model() {
    // One level (Lf == clev), one member of 5 nodes, fp64 inverse: the dense solve reads the
    // 15 x 15 inverse (8 * 225 = 1800) and b, writes x (16 * 15 = 240), the dot product reads both
    // again (240) = 2280, all of it on the "fine" level.  Launches: k_sell<kPcg>, k_fin, k_axpy,
    // k_fin, k_coarse, k_dot, k_fin = 7
    {
        MgpisBytes M;
        M.lev = {bytes_level({5}, {13}, {0})};
        bytes_check(M, 0, 2280.0, 0.0, 7, "one level");
        // the Krylov SpMV: 13 blocks of 72 B + 4 B column, and 5 vectors of 24 B per node
        pcheck(fine_kernel_bytes(M, 0) == 76.0 * 13 + 120.0 * 5, "one level: fine kernel bytes");
    }

    // Two levels under block Jacobi: fp64 copies (72 B + 4 B column per block, 9 * 8 = 72 B of inverse
    // per node), list transfers with stored weights, dense fp64 solve on level 0.  Members (fine
    // nodes n, coarse nodes c, fine blocks z, stencil entries t): 0 = (5, 2, 11, 7), 1 = (8, 3, 20, 12).
    // Per launch, nu = 1 (all on the fine level but the coarse solve):
    //   k_jac0      b in, x out, inverse: (48 + 72) n                  600       960
    //   residual    76 z + 72 n (x gathered, b, r)                    1196      2096
    //   restriction r_f 24 n + 12 t + (mask 1 + b_c 24) c              254       411
    //   coarse      8 (3c)^2 + 16 (3c)              [below]            384       792
    //   prolongat.  e_c 24 c + (mask 1 + x in/out 48) n + 12 t         377       608
    //   sweep       76 z + (x, b, x' 72 + inverse 72) n               1556      2672
    //                                                          fine   3983      6747
    // launches: the 5 of the recurrence + those 6 = 11.  nu = 2 adds one sweep going down and one
    // coming up: + 2 * 1556 = 7095, + 2 * 2672 = 12091, 13 launches
    auto two_level = [] {
        MgpisBytes M;
        M.lev = {bytes_level({2, 3}, {4, 9}, {0, 0}), bytes_level({5, 8}, {11, 20}, {7, 12})};
        M.smoother = 1;
        return M;
    };
    {
        MgpisBytes M = two_level();
        bytes_check(M, 0, 3983.0, 384.0, 11, "block Jacobi, nu 1");
        bytes_check(M, 1, 6747.0, 792.0, 11, "block Jacobi, nu 1");
        M.nu = 2;
        bytes_check(M, 0, 7095.0, 384.0, 13, "block Jacobi, nu 2");
        bytes_check(M, 1, 12091.0, 792.0, 13, "block Jacobi, nu 2");
        // a member's figures do not move with another member's counts
        M.lev[1].nloc[1] = 80, M.lev[1].nnzb_sub[1] = 200, M.lev[1].tent_sub[1] = 120, M.lev[0].nloc[1] = 30;
        bytes_check(M, 0, 7095.0, 384.0, 13, "block Jacobi, nu 2, other member changed");
        // operator bytes of a fine pass by storage type and column width (11 blocks)
        M = two_level();
        pcheck(fine_matrix_bytes(M, 0, kVal64) == 836.0 && fine_matrix_bytes(M, 0, kVal32) == 440.0 &&
                   fine_matrix_bytes(M, 0, kValH16) == 264.0 && fine_matrix_bytes(M, 0, kValQ8) == 176.0,
               "fine pass bytes by storage type");
        M.lev[1].col16 = true;
        pcheck(fine_matrix_bytes(M, 0, kVal64) == 814.0 && fine_matrix_bytes(M, 0, kVal64, false) == 836.0,
               "fine pass bytes with 16-bit columns");
    }
    // Chebyshev (smoother 2) on member 0: k_jac0 also writes d (+ 24 n = 120), the sweep reads and
    // writes d (+ 48 n = 240): 3983 + 360 = 4343
    {
        MgpisBytes M = two_level();
        M.smoother = 2;
        bytes_check(M, 0, 4343.0, 384.0, 11, "Chebyshev, two levels");
    }
    // Chebyshev on three levels, one member, (nodes, blocks, stencil entries) = level 0 (1, -, -),
    // 1 (3, 5, 4), 2 (6, 14, 9): the restriction onto level 1 fuses that level's first sweep
    //   fine   k_jac0 144 * 6 = 864; residual 76 * 14 + 72 * 6 = 1496; restriction 24 * 6 + 12 * 9 +
    //          (25 + inverse 72 + x_c 24 + d_c 24) * 3 = 687; prolongation 24 * 3 + 49 * 6 + 12 * 9 = 474;
    //          sweep 76 * 14 + 192 * 6 = 2216                                              = 5737
    //   below  residual 76 * 5 + 72 * 3 = 596; restriction 24 * 3 + 12 * 4 + 25 * 1 = 145; coarse
    //          8 * 9 + 16 * 3 = 120; prolongation 24 * 1 + 49 * 3 + 12 * 4 = 219; sweep 76 * 5 + 192 * 3 = 956
    //                                                                                      = 2036
    // launches: 5 + k_jac0 + 2 (residual, restriction) + coarse + 2 (prolongation, sweep) = 15
    {
        MgpisBytes M;
        M.lev = {bytes_level({1}, {1}, {0}), bytes_level({3}, {5}, {4}), bytes_level({6}, {14}, {9})};
        M.smoother = 2;
        bytes_check(M, 0, 5737.0, 2036.0, 15, "Chebyshev, three levels");
    }
    // Transfer forms against the lists, member 0 above (restriction 254, prolongation 377 of 3983):
    //   lattice   restriction 24 n + (25 + child mask and fine copy 8) c = 186, prolongation 24 c + 49 n
    //             + one 4-B word per fine node = 313                                  -> 3851
    //   uniform   restriction as the lists; prolongation reads 4 B per entry, no weight: 48 + 245 + 28 = 321
    //                                                                                 -> 3927
    //   2 block entries: restriction + 32 * 2 + b_c read and written again 24 c = + 112, prolongation
    //             + 32 * 2 = + 64                                                     -> 4159
    {
        MgpisBytes M = two_level();
        M.lev[1].lat = true;
        bytes_check(M, 0, 3851.0, 384.0, 11, "lattice transfer");
        M = two_level();
        M.lev[1].uw = true;
        bytes_check(M, 0, 3927.0, 384.0, 11, "uniform-weight transfer");
        M = two_level();
        M.lev[1].tblk_sub = {2, 0};
        bytes_check(M, 0, 4159.0, 384.0, 11, "block transfer entries");
        bytes_check(M, 1, 6747.0, 792.0, 11, "block transfer entries of the other member");
    }
    // Block Jacobi on fp32 iterate copies (x4), nu = 2, member 0 alone: fp32 copy with 16-bit columns
    // (38 B per block, 418 per pass), fp32 inverses (36 B per node, the dense one 4 B per entry)
    //   k_jac0 (b 24 + x4 16 + 36) n = 380; sweep 418 + (x4 16 + b 24 + x4' 16 + 36) n = 878; residual
    //   418 + (16 + 48) n = 738; restriction 254; prolongation 48 + (1 + 32) n + 84 = 297; sweep 878; last
    //   sweep writes fp64: 418 + (16 + 24 + 24 + 36) n = 918                              = 4343
    //   coarse 4 * 36 + 16 * 6 = 240
    {
        MgpisBytes M;
        M.lev = {bytes_level({2}, {4}, {0}), bytes_level({5}, {11}, {7})};
        M.smoother = 1, M.nu = 2, M.ainv32 = true;
        M.lev[1].vt = kVal32, M.lev[1].col16 = true, M.lev[1].x4 = true;
        bytes_check(M, 0, 4343.0, 240.0, 13, "block Jacobi on fp32 iterates");
    }

    // Colour Gauss-Seidel (smoother 3), K = 2 colours, one member: 6 fine and 2 coarse nodes, 8
    // stencil entries, 10 off-diagonal blocks in the fp32 copy with 16-bit columns (38 B each, 380 per
    // pass), fp32 inverses (36 B per row and 4 B per dense entry).  x gathered per row: 24 (K - 1) / 2
    // = 12 by the forward sweep and the residual, 24 (K - 1) = 24 by the backward sweep
    //   forward     380 + (b 24 + 36 + x 24 + row index 4 + 12) * 6 =  980
    //   residual    (r 24 + 4 + 12) * 6                             =  240
    //   restriction 24 * 6 + 12 * 8 + 25 * 2                        =  290
    //   coarse      4 * 36 + 16 * 6                         [below] =  240
    //   prolongat.  24 * 2 + (1 + 48) * 6 + 12 * 8                  =  438
    //   backward    380 + (24 + 36 + 24 + 4 + 24) * 6               = 1052     fine = 3000
    // launches: 5 + 2 forward + residual + restriction + coarse + prolongation + 2 backward = 13
    auto colours = [] {
        MgpisBytes M;
        M.lev = {bytes_level({2}, {4}, {0}), bytes_level({6}, {40}, {8})};
        M.lev[1].vt = kVal32, M.lev[1].col16 = true;
        M.smoother = 3, M.ainv32 = true;
        M.gs.ncol = 2, M.gs.vt = kVal32, M.gs.col16 = true;
        M.gs.nnzb_sub = {10};
        return M;
    };
    {
        MgpisBytes M = colours();
        bytes_check(M, 0, 3000.0, 240.0, 13, "colour Gauss-Seidel");
        // band mode: 4 band rows, 1 ring row with 3 band blocks, 1 far row
        //   x = 0, r = b outside the colours 76 * 2 = 152; forward 380 + 100 * 4 = 780; residual 40 * 4 =
        //   160; the ring's residual 38 * 3 + 76 * 1 = 190; restriction 290; prolongation 438; backward
        //   380 + 112 * 4 = 828; b . x outside the colours 52 * 2 = 104                   = 2942
        // launches: + the three launches outside the colours = 16
        M.gs.band = true;
        M.gs.band_rows_sub = {4}, M.gs.ring_rows_sub = {1}, M.gs.far_rows_sub = {1}, M.gs.ring_nnzb_sub = {3};
        bytes_check(M, 0, 2942.0, 240.0, 16, "colour Gauss-Seidel, band mode");
        // fp32 iterate and residual copies (x4, r4: 16 B where 24 B was) with the lattice transfer they need
        //   forward 380 + (24 + 36 + 16 + 4 + 8) * 6 = 908; residual (16 + 4 + 8) * 6 = 168; restriction
        //   16 * 6 + (25 + 8) * 2 = 162; prolongation 24 * 2 + (1 + 32) * 6 + 4 * 6 = 270; backward 380 +
        //   (24 + 36 + z 24 + x4 16 + 4 + 16) * 6 = 1100                                  = 2608
        // the residual left in fp64 (x4 only): residual (24 + 4 + 8) * 6 = 216, restriction 24 * 6 + 66 =
        //   210                                                                           = 2704
        M = colours();
        M.lev[1].lat = true, M.gs.x4 = true, M.gs.r4 = true;
        bytes_check(M, 0, 2608.0, 240.0, 13, "colour Gauss-Seidel on fp32 iterates and residual");
        M.gs.r4 = false;
        bytes_check(M, 0, 2704.0, 240.0, 13, "colour Gauss-Seidel on fp32 iterates");
    }
    // Colour SSOR (smoother 4) on the same shape: L and U passes of 190 each
    //   forward from zero  190 + (b 24 + 36 + x 24 + w 24 + 4 + 12) * 6 =  934
    //   backward           190 + (b, w 48 + 36 + x 24 + 4 + 12) * 6     =  934
    //   residual           190 + (w 24 + r 24 + 4 + 12) * 6             =  574
    //   restriction 290, prolongation 438
    //   forward            380 + (24 + 36 + 24 + 24 + 4 + 24) * 6       = 1196
    //   backward           190 + (48 + 36 + z 24 + 4 + 12) * 6          =  934     fine = 5300
    // launches: 5 + (2 + 2 + 1) + restriction + coarse + prolongation + (2 + 2) = 17
    {
        MgpisBytes M = colours();
        M.smoother = 4;
        bytes_check(M, 0, 5300.0, 240.0, 17, "colour SSOR");
    }

    // Table mode: a fine pass reads 4 B per block and per node and the member's share of the table
    // by nodes -- 3 row types of 27 doubles = 648 B over 4 + 12 nodes: 162 and 486, which sum to
    // the table; the share is the one figure that moves with another member's count
    {
        MgpisBytes M;
        M.lev = {bytes_level({1, 1}, {1, 1}, {0, 0}), bytes_level({4, 12}, {9, 30}, {0, 0})};
        M.lev[1].tbl = true, M.lev[1].ntypes = 3, M.lev[1].tstride = 27;
        const double a = fine_matrix_bytes(M, 0, kVal64), b = fine_matrix_bytes(M, 1, kVal64);
        pcheck(a == 36.0 + 16.0 + 162.0 && b == 120.0 + 48.0 + 486.0, "table mode: fine pass bytes");
        pcheck((a - 52.0) + (b - 168.0) == 648.0, "table mode: the shares sum to the table");
        M.lev[1].nloc[1] = 4;
        pcheck(fine_matrix_bytes(M, 0, kVal64) == 36.0 + 16.0 + 324.0, "table mode: the share follows the node total");
    }
    std::printf("{\"case\": \"mgpis_bytes\", \"tallies\": 18}\n");
}

void run_mgpis_plan() {
    plan_levels_and_records();
    plan_transfers_and_colours();
    byte_model();
}

// ---- the ADMM handle's host setup (admm_plan.cpp), called directly on established problems
void acheck(bool good, const std::string& what) {
    if (!good) {
        std::fprintf(stderr, "FAIL admm_plan: %s\n", what.c_str());
        ++g_fail;
    }
}

// what MgpisDevice would hold of the owned subdomains' batch, from the MGPIS plan alone
struct HostBatch {
    std::vector<SubdomainOps> ops;
    MgpisNumbering num;
    std::vector<int64_t> noff;  // fine level: first node per member
    BatchView V;                // (points into num)
    int64_t fine_dof(int s, int64_t d) const { return 3 * (noff[s] + num.perm.back()[s][d / 3]) + d % 3; }
};
std::unique_ptr<HostBatch> host_batch(const MCONTACT& mc, const std::vector<AdmmSub>& subs) {
    auto B = std::make_unique<HostBatch>();
    if (subs.empty()) return B;
    for (const auto& S : subs) B->ops.push_back(subdomain_ops(mc.multGrid[S.tv]));
    B->num = mgpis_numbering(B->ops, 0);
    const MgpisTuning tune;
    const int nlev = (int)B->ops[0].nnodes.size();
    std::vector<LevelShape> sh;
    for (int l = 0; l < nlev; ++l) sh.push_back(plan_level(B->ops, B->num, l, true, 0, tune));
    for (int l = 0; l < nlev; ++l) {
        BatchLevelView v;
        v.nn = sh[l].nn;
        v.noff = sh[l].noff;
        v.nloc = sh[l].nloc;
        if (l > 0) {
            const TransferShape t = plan_transfer(B->ops, B->num, l, sh[l], sh[l - 1], tune);
            v.tent_sub = t.tent_sub;
            v.lat = t.lat;
        }
        B->V.lev.push_back(v);
    }
    B->noff = sh.back().noff;
    B->V.level_perm = &B->num.perm;
    for (size_t s = 0; s < subs.size(); ++s)
        B->V.nfree.push_back((int64_t)free_dof_map(B->ops[s], B->num.perm[nlev - 1][s], B->noff[s]).size());
    return B;
}

double wval(int64_t i) { return std::sin(0.37 * (double)i) + 0.1 * std::cos(5.1 * (double)i) + 0.01; }

// a product formed term by term: the sum, the sum of magnitudes and the term count per row
struct Acc {
    std::vector<double> y, a;
    std::vector<int64_t> k;
    explicit Acc(int64_t n) : y(n, 0.0), a(n, 0.0), k(n, 0) {}
    void add(int64_t r, double v, double x) {
        y[r] += v * x;
        a[r] += std::fabs(v * x);
        ++k[r];
    }
    // |got - y| within (k - 1) eps sum |terms|: both sides sum the same products in another order
    bool close(int64_t r, double got) const {
        return std::fabs(got - y[r]) <= (double)std::max<int64_t>(k[r] - 1, 0) * 2.220446049250313e-16 * a[r];
    }
};

std::vector<double> sell_apply(const SellPlan& P, const std::vector<double>& W) {
    std::vector<double> y(P.nrow, 0.0);
    for (int64_t r = 0; r < P.nrow; ++r)
        for (int64_t q = P.off[r / 64]; q < P.off[r / 64] + P.slots[r / 64]; ++q) y[r] += P.val[q * 64 + r % 64] * W[P.col[q * 64 + r % 64]];
    return y;
}

// the packed operator against the term-by-term product; columns inside W; slots past a row's
// terms and rows past the product's hold column 0, value 0
void sell_check(const SellPlan& P, const Acc& ref, const std::vector<double>& W, const std::string& what) {
    const int64_t nw = (int64_t)W.size(), nr = (int64_t)ref.y.size();
    bool shape = P.nrow % 64 == 0 && P.nch == P.nrow / 64 && P.nrow >= nr && (int64_t)P.off.size() == P.nch + 1, cols = true, pads = true,
         prod = true;
    acheck(shape, what + ": padded rows, chunk count");
    if (!shape) return;
    const std::vector<double> y = sell_apply(P, W);
    for (int64_t r = 0; r < P.nrow; ++r) {
        const int64_t kr = r < nr ? ref.k[r] : 0;
        for (int64_t q = P.off[r / 64], j = 0; q < P.off[r / 64 + 1]; ++q, ++j) {
            const int32_t c = P.col[q * 64 + r % 64];
            cols = cols && c >= 0 && c < nw;
            if (j >= kr) pads = pads && c == 0 && P.val[q * 64 + r % 64] == 0.0;
        }
        if (r < nr) prod = prod && ref.close(r, y[r]);
    }
    acheck(cols, what + ": every column inside W");
    acheck(pads, what + ": pad slots hold column 0, value 0");
    acheck(prod, what + ": the packed product equals the term-by-term product within (k - 1) eps sum |terms|");
}

struct AdmmCase {
    ddpca_problem_t p = nullptr;
    Problem* P = nullptr;
    std::vector<int32_t> owner;
    int rank = 0;
    std::unique_ptr<HostBatch> B;
    AdmmTables T;
    ~AdmmCase() {
        if (p) ddpca_problem_destroy(p);
    }
};

// tables of (problem, owner, rank) with the layout checks
void plan_case_tables(AdmmCase& c, const AdmmTuning& tune, const std::string& name) {
    const MCONTACT& mc = c.P->mc;
    std::vector<AdmmSub> subs = owned_subdomains(*c.P, c.owner, c.rank);
    c.B = host_batch(mc, subs);
    c.T = plan_tables(mc, subs, c.owner, c.rank, c.B->V, tune);
    const AdmmTables& T = c.T;
    // regions: 64-aligned, in order, disjoint
    bool lay = T.oH == T.NU && T.oS == T.oH + T.NH && T.oG == T.oS + 2 * T.R && T.G >= 64;
    for (int64_t v : {T.NU, T.NH, T.R, T.G, T.oH, T.oS, T.oG}) lay = lay && v % 64 == 0 && v >= 0;
    std::vector<std::pair<int64_t, int64_t>> useg, hseg, rseg, gseg;
    for (const auto& S : T.subs) {
        useg.push_back({S.dof0, S.dof0 + 3 * S.nn});
        hseg.push_back({S.hoff, S.hoff + S.nh});
        lay = lay && c.owner[S.tv] == c.rank && S.nn == mc.multGrid[S.tv].leveCount.back();
    }
    int64_t nside = 0;
    for (int64_t ts = 0; ts < T.nint; ++ts)
        for (int s = 0; s < 2; ++s) nside += c.owner[mc.searCont[ts].body[s]] == c.rank;
    lay = lay && (int64_t)T.sides.size() == nside && (int64_t)T.itfs.size() == T.nint;
    for (const auto& sd : T.sides) {
        rseg.push_back({sd.roff, sd.roff + sd.m});
        lay = lay && sd.roff % 64 == 0 && sd.tv == mc.searCont[sd.ts].body[sd.s] && c.owner[sd.tv] == c.rank && T.subs[sd.sub].tv == sd.tv;
    }
    int64_t last_cross = -1, first_local = INT64_MAX;
    for (const auto& I : T.itfs) {
        gseg.push_back({I.goff, I.goff + I.mip});
        const Interface& itf = mc.searCont[I.ts];
        const bool cross = c.owner[itf.body[0]] != c.owner[itf.body[1]];
        lay = lay && I.cross == cross && I.mine == (c.owner[itf.body[0]] == c.rank || c.owner[itf.body[1]] == c.rank) && I.mip == itf.mip();
        if (cross) last_cross = std::max(last_cross, I.goff);
        else first_local = std::min(first_local, I.goff);
    }
    lay = lay && last_cross < first_local;  // cross-rank interfaces first
    auto disjoint = [](std::vector<std::pair<int64_t, int64_t>> v, int64_t n) {
        std::sort(v.begin(), v.end());
        int64_t end = 0;
        for (const auto& s : v) {
            if (s.first < end || s.second > n) return false;
            end = s.second;
        }
        return true;
    };
    lay = lay && disjoint(useg, T.NU) && disjoint(hseg, T.NH) && disjoint(rseg, T.R) && disjoint(gseg, T.G);
    acheck(lay, name + ": W's regions are 64-aligned and disjoint, the tables name the owned sides");
    std::vector<int32_t> on = T.onode;
    std::sort(on.begin(), on.end());
    bool perm = true;
    for (size_t i = 0; i < on.size(); ++i) perm = perm && on[i] == (int32_t)i;
    acheck(perm && (int64_t)T.cf.size() == T.NU && (int64_t)T.presc.size() == T.NU, name + ": onode is a permutation");
    bool mx = T.maxit.size() == T.subs.size();
    for (size_t i = 0; mx && i < T.subs.size(); ++i) mx = T.maxit[i] == mc.multGrid[T.subs[i].tv].freeCount.back();
    acheck(mx, name + ": maxit is the free dof count");
}

// every interface operator of the case, applied to a pseudo-random W
void plan_case_operators(AdmmCase& c, const std::string& name) {
    const MCONTACT& mc = c.P->mc;
    const AdmmTables& T = c.T;
    const HostBatch& B = *c.B;
    std::vector<double> W(T.oG + T.G);
    for (size_t i = 0; i < W.size(); ++i) W[i] = wval((int64_t)i);
    auto wc = [&](const AdmmSub& S, int64_t col) { return col < 3 * S.nn ? S.dof0 + col : T.oH + S.hoff + (col - 3 * S.nn); };
    Acc gam(T.G), aux(T.R), lam(T.R), wv(2 * T.R), hang(T.NH), cpl(std::max<int64_t>(T.NU, 1));
    std::vector<double> gc(T.G, 0.0), ri(std::max<int64_t>(T.R, 1), 0.0);
    for (const auto& sd : T.sides) {
        const Interface& itf = mc.searCont[sd.ts];
        const AdmmItf& I = T.itfs[sd.ts];
        const AdmmSub& S = T.subs[sd.sub];
        const int s = (int)sd.s;
        const int64_t aux0 = T.oS + sd.roff, lam0 = T.oS + T.R + sd.roff, g0 = T.oG + I.goff;
        const double half = s == 0 ? 0.5 : -0.5;
        for (int64_t i = 0; i < itf.mip(); ++i) {
            if (!itf.factored) {
                for (int64_t k = itf.inpoLagr[s].ptr[i]; k < itf.inpoLagr[s].ptr[i + 1]; ++k)
                    gam.add(I.goff + i, half * itf.inpoLagr[s].val[k], W[lam0 + itf.inpoLagr[s].col[k]]);
                for (int64_t k = itf.pemaInpo_r[s].ptr[i]; k < itf.pemaInpo_r[s].ptr[i + 1]; ++k)
                    gam.add(I.goff + i, half * itf.pemaInpo_r[s].val[k], W[wc(S, itf.pemaInpo_r[s].col[k])]);
            }
            if (s == 0) gc[I.goff + i] = -0.5 * (itf.pemaDiag[i] * itf.inpoNgap[i]);
        }
        // T^T u without forming the transpose: body dof j, side row c
        for (int pena = 0; pena < 2; ++pena) {
            const Csr& A = pena ? itf.systTran_pena[s] : itf.systTran[s];
            for (int64_t j = 0; j < A.nrow; ++j)
                for (int64_t k = A.ptr[j]; k < A.ptr[j + 1]; ++k) {
                    if (pena) {
                        aux.add(sd.roff + A.col[k], A.val[k], W[wc(S, j)]);
                        lam.add(sd.roff + A.col[k], A.val[k], W[wc(S, j)]);
                    } else {
                        wv.add(sd.roff + A.col[k], A.val[k], W[wc(S, j)]);
                    }
                }
        }
        for (int64_t r = 0; r < itf.mside(s); ++r) {
            for (int64_t k = itf.inteMass[s].ptr[r]; k < itf.inteMass[s].ptr[r + 1]; ++k)
                aux.add(sd.roff + r, itf.inteMass[s].val[k], W[lam0 + itf.inteMass[s].col[k]]);
            for (int64_t k = itf.inteInpo[s].ptr[r]; k < itf.inteInpo[s].ptr[r + 1]; ++k) {
                aux.add(sd.roff + r, itf.inteInpo[s].val[k], W[g0 + itf.inteInpo[s].col[k]]);
                if (!itf.factored) wv.add(T.R + sd.roff + r, itf.inteInpo[s].val[k], W[g0 + itf.inteInpo[s].col[k]]);
            }
            for (int64_t k = itf.inteMass_pena[s].ptr[r]; k < itf.inteMass_pena[s].ptr[r + 1]; ++k)
                lam.add(sd.roff + r, -itf.inteMass_pena[s].val[k], W[aux0 + itf.inteMass_pena[s].col[k]]);
            ri[sd.roff + r] = 1.0 / itf.penN;
        }
        // coupling rows: [systTran_pena | -systTran] on the free dofs, hanging rows through hangProl
        const MULTIGRID& g = mc.multGrid[sd.tv];
        const Csr& Tp = itf.systTran_pena[s];
        const Csr& Tr = itf.systTran[s];
        for (int64_t r = 0; r < Tp.nrow; ++r) {
            std::vector<std::pair<int64_t, double>> tgt;
            if (r < 3 * S.nn) tgt.push_back({r, 1.0});
            else
                for (int64_t k = g.hangProl.ptr[r - 3 * S.nn]; k < g.hangProl.ptr[r - 3 * S.nn + 1]; ++k)
                    tgt.push_back({g.hangProl.col[k], g.hangProl.val[k]});
            for (const auto& t : tgt) {
                if (!g.consFlag[t.first] || t.second == 0.0) continue;
                const int64_t row = B.fine_dof(sd.sub, t.first);
                for (int64_t k = Tp.ptr[r]; k < Tp.ptr[r + 1]; ++k) cpl.add(row, t.second * Tp.val[k], W[aux0 + Tp.col[k]]);
                for (int64_t k = Tr.ptr[r]; k < Tr.ptr[r + 1]; ++k) cpl.add(row, -t.second * Tr.val[k], W[lam0 + Tr.col[k]]);
            }
        }
    }
    int64_t nhang = 0;
    for (const auto& S : T.subs) {
        const Csr& Hp = mc.multGrid[S.tv].hangProl;
        nhang += S.nh;
        for (int64_t r = 0; r < S.nh; ++r)
            for (int64_t k = Hp.ptr[r]; k < Hp.ptr[r + 1]; ++k) hang.add(S.hoff + r, Hp.val[k], W[wc(S, Hp.col[k])]);
    }
    // ---- the planned operators
    const AdmmOperators O = plan_operators(mc, T, false);
    {
        // gamma = the side-0 rows plus the rank-local side-1 halves scattered onto them
        std::vector<double> y = sell_apply(O.gamma, W);
        bool dst = true;
        if (O.has_gamma1) {
            const std::vector<double> y1 = sell_apply(O.gamma1, W);
            for (size_t j = 0; j < O.gam1_dst.size(); ++j) {
                dst = dst && O.gam1_dst[j] >= 0 && O.gam1_dst[j] < T.G;
                if (dst) y[O.gam1_dst[j]] += y1[j];
            }
            for (int32_t cc : O.gamma1.col) dst = dst && cc >= 0 && cc < (int32_t)W.size();
        }
        bool prod = (int64_t)y.size() == T.G;
        for (int64_t r = 0; prod && r < T.G; ++r) prod = gam.close(r, y[r]);
        for (int32_t cc : O.gamma.col) dst = dst && cc >= 0 && cc < (int32_t)W.size();
        acheck(dst && prod, name + ": gamma halves equal +-1/2 (inpoLagr lambda + pemaInpo_r u)");
        acheck(O.gcst == gc, name + ": gamma's constant part");
    }
    sell_check(O.aux, aux, W, name + " op_aux");
    sell_check(O.lam, lam, W, name + " op_lam");
    const AdmmOperators Of = plan_operators(mc, T, true);
    acheck(Of.aux.nch == 0 && Of.lam.nch == 0 && Of.gamma.col == O.gamma.col && Of.gamma.val == O.gamma.val,
           name + ": the fused update plans no aux / lambda rows, the same gamma");
    if (!T.sides.empty()) {
        const AdmmFused F = plan_fused(mc, T);
        sell_check(F.wv, wv, W, name + " op_wv");
        acheck(F.rinv == ri, name + ": rinv = 1 / penN on the sides' rows");
    }
    for (int which = 0; which < 3; ++which) {
        const MassList L = mass_list(mc, T, which);
        bool good = L.A.size() == (which == 2 ? 2 : 1) * T.sides.size() && L.roff.size() == L.A.size() && L.nrow == (which == 2 ? 2 : 1) * T.R;
        for (size_t i = 0; good && i < L.A.size(); ++i) {
            const AdmmSide& sd = T.sides[i % T.sides.size()];
            const Interface& itf = mc.searCont[sd.ts];
            good = L.A[i] == (which == 0 ? &itf.inteMass_pena[sd.s] : &itf.inteMass[sd.s]) &&
                   L.roff[i] == sd.roff + (int64_t)(i / T.sides.size()) * T.R;
        }
        acheck(good, name + ": the mass batches' systems and row offsets");
    }
    {
        const CouplingPlan K = plan_coupling(mc, T, B.V);
        bool good = K.cptr.size() == K.crow.size() + 1 && K.ccol.size() == K.cval.size(), rows = true;
        std::vector<char> seen(cpl.y.size(), 0);
        for (size_t i = 0; good && i < K.crow.size(); ++i) {
            double y = 0.0;
            for (int64_t k = K.cptr[i]; k < K.cptr[i + 1]; ++k) {
                good = good && K.ccol[k] >= T.oS && K.ccol[k] < T.oG && (k == K.cptr[i] || K.ccol[k] > K.ccol[k - 1]);
                if (good) y += K.cval[k] * W[K.ccol[k]];
            }
            good = good && K.crow[i] >= 0 && K.crow[i] < T.NU && !seen[K.crow[i]] && cpl.close(K.crow[i], y);
            if (good) seen[K.crow[i]] = 1;
        }
        for (size_t r = 0; r < cpl.y.size(); ++r) rows = rows && (seen[r] != 0) == (cpl.k[r] > 0);
        acheck(good, name + ": coupling rows equal [systTran_pena | -systTran] folded through hangProl, columns merged");
        acheck(rows, name + ": a coupling row for every coupled free dof and no other");
    }
    if (T.NH) sell_check(plan_hanging(mc, T), hang, W, name + " op_hang");
    // factored per-ip operands: indices inside W's lambda / u regions, shape values as the ips'
    int64_t nfact = 0;
    for (const AdmmItf& I : T.itfs) {
        const Interface& itf = mc.searCont[I.ts];
        if (!I.mine || !itf.factored) continue;
        ++nfact;
        const FactItfPlan F = plan_factored(mc, T, I);
        bool good = F.nip == (int64_t)itf.ip.size() && F.C == itf.comp() && F.goff == I.goff;
        for (int s = 0; s < 2 && good; ++s) {
            good = (F.own[s] != 0) == (c.owner[itf.body[s]] == c.rank);
            if (!F.own[s]) continue;
            const AdmmSide& sd = T.sides[T.side_of.at({I.ts, s})];
            const AdmmSub& S = T.subs[sd.sub];
            for (int64_t q = 0; q < F.nip && good; ++q)
                for (int a = 0; a < 4 && good; ++a) {
                    const int64_t node = itf.ip[q].node[s][a];
                    const auto at = std::find(itf.nodeCont[s].begin(), itf.nodeCont[s].end(), node) - itf.nodeCont[s].begin();
                    good = F.M[s][a * F.nip + q] == itf.ip[q].shap[s][a] && F.lam[s][a * F.nip + q] == T.oS + T.R + sd.roff + F.C * at &&
                           F.u[s][a * F.nip + q] == wc(S, 3 * node);
                }
            good = good && F.nnc[s] == (int64_t)itf.nodeCont[s].size() && F.nptr[s].size() == (size_t)F.nnc[s] + 1 &&
                   F.nptr[s].back() == 4 * F.nip && F.roff[s] == sd.roff;
        }
        acheck(good, name + ": factored per-ip operands index the side's lambda and the body's u");
    }
    std::printf("{\"case\": \"admm_plan\", \"problem\": \"%s\", \"rank\": %d, \"W\": %lld, \"sides\": %zu, \"factored\": %lld, \"hanging_dofs\": %lld}\n",
                name.c_str(), c.rank, (long long)W.size(), T.sides.size(), (long long)nfact, (long long)nhang);
}

std::unique_ptr<AdmmCase> admm_case(const char* kind, const std::vector<double>& params, int64_t musc, int ranks, int rank,
                                    const std::vector<int32_t>* owner_in = nullptr) {
    auto c = std::make_unique<AdmmCase>();
    ok(ddpca_problem_create(kind, params.data(), (int)params.size(), &c->p), kind);
    if (!c->p) return nullptr;
    c->P = reinterpret_cast<Problem*>(c->p);
    const int64_t nsub = (int64_t)c->P->mc.multGrid.size();
    std::vector<int64_t> dole(nsub, 1);
    if (musc) ok(ddpca_problem_set_coarse(c->p, musc, dole.data()), "set_coarse");
    c->owner.assign(nsub, 0);
    for (int64_t tv = 0; tv < nsub; ++tv) c->owner[tv] = owner_in ? (*owner_in)[tv] : (int32_t)(tv * ranks / nsub);
    c->rank = rank;
    if (ranks == 1) ok(ddpca_problem_establish(c->p), "establish");
    else ok(ddpca_problem_establish_owned(c->p, c->owner.data(), rank), "establish_owned");
    return c;
}

// which (region, subdomain or side, local index) a workspace column is
std::array<int64_t, 3> locate(const AdmmTables& T, int64_t w) {
    if (w < T.oH) {
        for (const auto& S : T.subs)
            if (w >= S.dof0 && w < S.dof0 + 3 * S.nn) return {0, S.tv, w - S.dof0};
    } else if (w < T.oS) {
        for (const auto& S : T.subs)
            if (w >= T.oH + S.hoff && w < T.oH + S.hoff + S.nh) return {0, S.tv, 3 * S.nn + (w - T.oH - S.hoff)};
    } else if (w < T.oG) {
        const int64_t half = w < T.oS + T.R ? 0 : 1, r = w - T.oS - half * T.R;
        for (const auto& sd : T.sides)
            if (r >= sd.roff && r < sd.roff + sd.m) return {1 + half, 2 * sd.ts + sd.s, r - sd.roff};
    }
    return {-1, -1, -1};
}

// the coarse right-hand side's slots of an R-rank layout against the one-rank plan
void coarse_rank_invariance(const char* kind, const std::vector<double>& params, int64_t musc, const std::vector<int32_t>& owner,
                            int ranks, const std::string& name) {
    const AdmmTuning tune;
    auto one = admm_case(kind, params, musc, 1, 0);
    if (!one) return;
    plan_case_tables(*one, tune, name + " r1");
    const CoarseRhsPlan R1 = plan_coarse_rhs(one->P->mc, one->T);
    const CoarseSpace& cs1 = one->P->mc.coarse;
    const int64_t n = cs1.n;
    // the row's own subdomain (none for LATIN's contact rows)
    std::vector<int64_t> row_tv(n, -1);
    for (int64_t tv = 0; tv + 1 < (int64_t)cs1.baseReco.size(); ++tv)
        for (int64_t r = cs1.baseReco[tv]; r < cs1.baseReco[tv + 1]; ++r) row_tv[r] = tv;
    bool sp = true, vals = true, cols = true, empty = true, f0 = true, srcs = true;
    int64_t nonempty = 0;
    for (int rank = 0; rank < ranks; ++rank) {
        auto c = admm_case(kind, params, musc, ranks, rank, &owner);
        if (!c) return;
        plan_case_tables(*c, tune, name + " rank " + std::to_string(rank));
        const CoarseRhsPlan R = plan_coarse_rhs(c->P->mc, c->T);
        sp = sp && R.slots.sptr == R1.slots.sptr && R.nslot == R1.nslot;
        srcs = srcs && R.slots.srcs == R1.slots.srcs;
        if (!sp || !srcs) break;
        for (int64_t r = 0; r < n; ++r)
            for (int64_t j = 0; j < (int64_t)R.slots.srcs[r].size(); ++j) {
                const int64_t q = R.slots.sptr[r] + j, tv = R.slots.srcs[r][j];
                const int64_t b = R.rptr[q], e = R.rptr[q + 1], b1 = R1.rptr[q], e1 = R1.rptr[q + 1];
                if (owner[tv] != rank) {
                    empty = empty && b == e && R.f0[q] == 0.0;
                    continue;
                }
                vals = vals && e - b == e1 - b1;
                for (int64_t k = 0; vals && k < e - b; ++k) {
                    vals = std::memcmp(&R.rval[b + k], &R1.rval[b1 + k], sizeof(double)) == 0;
                    const auto at = locate(c->T, R.rcol[b + k]);
                    cols = cols && at[0] >= 0 && at == locate(one->T, R1.rcol[b1 + k]);
                }
                nonempty += e > b;
                // globForc_1 in the row's own slot on its owner, zero in every other slot
                f0 = f0 && (tv == row_tv[r] ? std::memcmp(&R.f0[q], &R1.f0[q], sizeof(double)) == 0 && R1.f0[q] == cs1.globForc_1[r]
                                            : R.f0[q] == 0.0 && R1.f0[q] == 0.0);
            }
    }
    acheck(sp && srcs, name + ": sptr and the slots' sources are the same on every rank");
    acheck(vals && nonempty > 0, name + ": the owner's value sequence of every slot equals the one-rank plan's bitwise");
    acheck(cols, name + ": every column maps back to the same (subdomain or side, local column)");
    acheck(empty, name + ": a non-owner's slot is empty");
    acheck(f0, name + ": f0 is non-zero only in the row's own slot on its owner");
    std::printf("{\"case\": \"admm_plan_rank_invariance\", \"problem\": \"%s\", \"ranks\": %d, \"rows\": %lld, \"slots\": %lld, \"filled\": %lld}\n",
                name.c_str(), ranks, (long long)n, (long long)R1.nslot, (long long)nonempty);
}

// DOUBLE_M(_1): forced by the row threshold; the hierarchy's numbering restated level by level
void coarse_mg_case(const char* kind, const std::vector<double>& params, int64_t musc, const std::string& name) {
    auto c = admm_case(kind, params, musc, 1, 0);
    if (!c) return;
    MCONTACT& mc = c->P->mc;
    const CoarseSpace& cs = mc.coarse;
    AdmmTuning tune;
    acheck(!coarse_solve_choice(cs, cs.n, 1, tune).mg, name + ": the dense solve by default");
    tune.coarse_mg_min = 1;
    const CoarseSolveChoice ch = coarse_solve_choice(cs, cs.n, 1, tune);
    acheck(ch.mg && !ch.mg_gather && ch.dense_bytes == 8.0 * (double)cs.n * (double)cs.n, name + ": a row threshold of 1 takes the multigrid solve");
    const MgPlan PL = plan_coarse_mg(mc, cs.n);
    const int64_t Lc = (int64_t)PL.nglob.size() - 1, nsub = (int64_t)mc.multGrid.size();
    bool mono = Lc == *std::max_element(mc.doleMcsc.begin(), mc.doleMcsc.end()) && PL.latin == cs.latin, ident = (int64_t)PL.S.size() == Lc;
    for (int64_t l = 1; l <= Lc; ++l) mono = mono && PL.nglob[l] >= PL.nglob[l - 1];
    for (int64_t l = 1; ident && l <= Lc; ++l) {
        const Stencil& S = PL.S[l - 1];
        ident = S.nf == PL.nglob[l] && S.nc == PL.nglob[l - 1] && (int64_t)S.ptr.size() == S.nf + 1;
        for (int64_t i = 0; ident && i < PL.nglob[l - 1]; ++i) ident = S.ptr[i + 1] - S.ptr[i] == 1 && S.col[S.ptr[i]] == i && S.w[S.ptr[i]] == 1.0;
        for (int32_t cc : S.col) ident = ident && cc >= 0 && cc < S.nc;
    }
    acheck(mono, name + ": nglob is non-decreasing");
    acheck(ident, name + ": the rows of a level's carried nodes are identity rows");
    std::vector<int32_t> f = PL.fdg;
    std::sort(f.begin(), f.end());
    bool inj = (int64_t)f.size() == cs.n && std::adjacent_find(f.begin(), f.end()) == f.end();
    for (int32_t d : PL.fdg) inj = inj && d >= 0 && d < 3 * PL.nglob[Lc] && PL.flev[Lc][d] == 1;
    acheck(inj, name + ": fdg is injective and lands on dofs flagged free at Lc");
    // level l = level l - 1's nodes, then every subdomain's new nodes in order (then LATIN's new
    // contact nodes): a subdomain node's flags are its consFlag
    bool pre = (int64_t)PL.flev.size() == Lc + 1;
    std::vector<std::vector<int64_t>> gid(nsub);
    for (int64_t l = 0; pre && l <= Lc; ++l) {
        int64_t cnt = l ? PL.nglob[l - 1] : 0;
        for (int64_t tv = 0; tv < nsub; ++tv) {
            const int64_t lv = std::max<int64_t>(0, mc.doleMcsc[tv] - (Lc - l));
            while ((int64_t)gid[tv].size() < mc.multGrid[tv].leveCount[lv]) gid[tv].push_back(cnt++);
            for (size_t j = 0; pre && j < gid[tv].size(); ++j)
                for (int a = 0; a < 3; ++a) pre = gid[tv][j] < PL.nglob[l] && PL.flev[l][3 * gid[tv][j] + a] == mc.multGrid[tv].consFlag[3 * j + a];
        }
        pre = pre && cnt <= PL.nglob[l] && (cs.latin || cnt == PL.nglob[l]) && (int64_t)PL.flev[l].size() == 3 * PL.nglob[l];
    }
    acheck(pre, name + ": flev[l] on a subdomain's nodes is its consFlag prefix");
    // refused: baseReco not matching the free dofs
    mc.coarse.baseReco[1] += 1;
    bool thrown = false;
    try {
        plan_coarse_mg(mc, cs.n);
    } catch (const ApiError& e) {
        thrown = e.code == DDPCA_EINVAL;
    }
    mc.coarse.baseReco[1] -= 1;
    acheck(thrown, name + ": baseReco not matching the free dofs is refused");
    std::printf("{\"case\": \"admm_plan_coarse_mg\", \"problem\": \"%s\", \"levels\": %lld, \"nodes\": %lld, \"rows\": %lld}\n", name.c_str(),
                (long long)(Lc + 1), (long long)PL.nglob[Lc], (long long)cs.n);
}

// the coarse tables of one case: assembled / factored prolongation inside their ranges
void plan_case_coarse(AdmmCase& c, const std::string& name, bool want_csr_rows) {
    const MCONTACT& mc = c.P->mc;
    const CoarseSpace& cs = mc.coarse;
    const AdmmTables& T = c.T;
    const CoarseRhsPlan R = plan_coarse_rhs(mc, T);
    bool rhs = (int64_t)R.rptr.size() == R.nslot + 1 && (int64_t)R.slots.sptr.size() == cs.n + 1 && (int64_t)R.f0.size() == std::max<int64_t>(R.nslot, 1);
    for (int64_t k = 0; rhs && k < R.rptr.back(); ++k) rhs = R.rcol[k] >= 0 && R.rcol[k] < T.oG;
    acheck(rhs, name + ": the coarse right-hand side's columns lie in u, aux and lambda");
    const int64_t nown = (int64_t)R.own_rows.size();
    const std::vector<double> dense = coarse_dense_rows(cs, R.own_rows, c.rank);
    bool dn = (int64_t)dense.size() == cs.n * cs.n;
    for (int64_t r : R.own_rows)
        for (int64_t k = cs.globCoup_1.ptr[r]; dn && k < cs.globCoup_1.ptr[r + 1]; ++k) dn = dense[r * cs.n + cs.globCoup_1.col[k]] == cs.globCoup_1.val[k];
    acheck(dn, name + ": the dense rows hold globCoup_1's owned rows");
    if (T.subs.empty() || cs.latin) return;
    const CoarseProlongPlan Q = cs.assembled ? plan_prolong_assembled(mc, T, R.xoff) : plan_prolong_factored(mc, T, c.B->V, R.slots, R.xoff);
    bool pr = (int64_t)Q.pptr.size() == Q.npr + 1 || (Q.npr == 0 && Q.pptr.size() == 1);
    for (int64_t r = 0; pr && r < Q.npr; ++r) {
        pr = Q.ptgt[r] >= 0 && Q.ptgt[r] < T.NU;
        for (int64_t k = Q.pptr[r]; pr && k < Q.pptr[r + 1]; ++k) pr = Q.pcol[k] >= 0 && Q.pcol[k] < nown;
    }
    if (!cs.assembled) {
        pr = pr && (int64_t)Q.qcol.size() == 8 * Q.qnn && (int64_t)Q.xsrc.size() == std::max<int64_t>(Q.nxn, 1) && (int64_t)Q.flag.size() == T.NU;
        for (int32_t q : Q.qcol) pr = pr && q >= -1 && q + 2 < Q.nxn;
        for (int32_t x : Q.xsrc) pr = pr && x >= -1 && x < nown;
        int64_t krows = 0;
        for (const auto& g : Q.kg) {
            pr = pr && g.rows.size() == g.src.size() && g.level >= Q.dmin && g.level < (int)c.B->V.lev.size();
            for (size_t i = 0; pr && i < g.rows.size(); ++i) pr = g.rows[i] >= 0 && g.rows[i] < R.nslot && g.src[i] >= 0 && g.src[i] < 3 * c.B->V.lev[g.level].nn;
            krows += (int64_t)g.rows.size();
        }
        pr = pr && krows == nown;  // every owned coarse row takes its stiffness part once
    }
    acheck(pr, name + ": the prolongation tables and gather groups stay inside xc, xn, u and the slots");
    if (want_csr_rows) acheck(Q.npr > 0, name + ": a rotated node takes the CSR branch of the factored prolongation");
    std::printf("{\"case\": \"admm_plan_coarse\", \"problem\": \"%s\", \"rank\": %d, \"own_rows\": %lld, \"csr_rows\": %lld, \"groups\": %zu}\n",
                name.c_str(), c.rank, (long long)nown, (long long)Q.npr, Q.kg.size());
}

void run_admm_plan() {
    AdmmTuning tune;
    // the two-block contact, frictionless and Coulomb, muscSett 0 / 1 (LATIN) / 2; each once as built
    // (factored per-ip operators) and once with the operators taken as a caller's (SELL gamma rows)
    for (double fric : {0.0, 0.3})
        for (int64_t musc : {0, 1, 2})
            for (int as_callers = 0; as_callers < 2; ++as_callers) {
                auto c = admm_case("twoblock", {fric, 2}, musc, 1, 0);
                if (!c) continue;
                if (as_callers)
                    for (auto& itf : c->P->mc.searCont) itf.factored = false;
                const std::string name = std::string("twoblock comp ") + (fric == 0.0 ? "1" : "3") + " musc " + std::to_string(musc) +
                                         (as_callers ? " (caller's operators)" : "");
                plan_case_tables(*c, tune, name);
                plan_case_operators(*c, name);
                if (musc) plan_case_coarse(*c, name, false);
                if (!as_callers) {
                    // both branches of the fused decision
                    AdmmTuning off;
                    off.mass_fused = false;
                    const bool fu = fused_update(c->P->mc, c->T, tune);
                    acheck(fu && !fused_update(c->P->mc, c->T, off), name + ": fused by default (proportional penalty operators), sequential with the flag off");
                    Interface& itf = c->P->mc.searCont[0];
                    const double keep = itf.inteMass_pena[0].val[0];
                    itf.inteMass_pena[0].val[0] *= 1.0 + 1e-9;
                    acheck(!fused_update(c->P->mc, c->T, tune), name + ": a penalty mass entry off the multiple ends the fused update");
                    itf.inteMass_pena[0].val[0] = keep;
                }
            }
    // the synthetic chain at its smallest: one rank, and two ranks with a cross-rank and a rank-local
    // interface on each (owner [0, 0, 1, 1]: the contacts rank-local, the glued links across)
    const std::vector<double> chain = {2, 2, 2, 1, 2, 0.3};
    for (int64_t musc : {2, 1}) {
        const std::vector<int32_t> owner = {0, 0, 1, 1};
        for (int ranks : {1, 2})
            for (int rank = 0; rank < ranks; ++rank)
                for (int as_callers = 0; as_callers < 2; ++as_callers) {
                    auto c = admm_case("dehw", chain, musc, ranks, rank, ranks == 2 ? &owner : nullptr);
                    if (!c) continue;
                    if (as_callers)
                        for (auto& itf : c->P->mc.searCont) itf.factored = false;
                    const std::string name = "chain musc " + std::to_string(musc) + " ranks " + std::to_string(ranks) + (as_callers ? " (caller's operators)" : "");
                    plan_case_tables(*c, tune, name);
                    plan_case_operators(*c, name);
                    if (!as_callers) plan_case_coarse(*c, name, false);
                }
        coarse_rank_invariance("dehw", chain, musc, owner, 2, "chain musc " + std::to_string(musc));
        coarse_mg_case("dehw", chain, musc, std::string("chain ") + (musc == 2 ? "DOUBLE_M_1" : "LATIN DOUBLE_M"));
    }
    coarse_rank_invariance("dehw", chain, 2, {0, 1, 0, 1}, 2, "chain musc 2, contacts across the ranks");
    // the chain's general mesh (contact band refined once more: a hanging level; rotated support nodes)
    {
        auto c = admm_case("dehw", {2, 2, 2, 1, 2, 0.3, 0, 0, 1, 1}, 2, 1, 0);
        if (c) {
            plan_case_tables(*c, tune, "general chain");
            int64_t nh = 0;
            for (const auto& S : c->T.subs) nh += S.nh;
            acheck(nh > 0 && c->T.NH >= nh, "general chain: a hanging level");
            plan_case_operators(*c, "general chain");
            for (auto& itf : c->P->mc.searCont) itf.factored = false;
            plan_case_operators(*c, "general chain (caller's operators)");
            plan_case_coarse(*c, "general chain", false);
        }
    }
    // a rank that owns nothing: the empty view, NU = 64, empty tables
    {
        const std::vector<int32_t> owner = {1, 1, 1, 1};
        auto c = admm_case("dehw", chain, 2, 2, 0, &owner);
        if (c) {
            plan_case_tables(*c, tune, "rank without subdomains");
            acheck(c->B->V.empty() && c->T.NU == 64 && c->T.NH == 0 && c->T.R == 0 && c->T.subs.empty() && c->T.sides.empty(),
                   "rank without subdomains: NU = 64, empty tables");
            plan_case_operators(*c, "rank without subdomains");
            const CoarseRhsPlan R = plan_coarse_rhs(c->P->mc, c->T);
            acheck(R.own_rows.empty() && R.rptr.back() == 0, "rank without subdomains: empty coarse slots");
        }
    }
    // refusals
    {
        auto c = admm_case("dehw", chain, 2, 1, 0);
        if (c) {
            plan_case_tables(*c, tune, "refusals");
            CoarseSpace& cs = c->P->mc.coarse;
            // subdomains 0 and 3 share no interface: an entry of subdomain 0 in a row of subdomain 3
            bool graph = true;
            for (const auto& itf : c->P->mc.searCont) graph = graph && !((itf.body[0] == 0 && itf.body[1] == 3) || (itf.body[0] == 3 && itf.body[1] == 0));
            acheck(graph, "refusals: subdomains 0 and 3 are no interface mates");
            Csr& A = cs.globTran_S[0];
            const Csr keep = A;
            const int64_t r = cs.baseReco[3];
            A.col.insert(A.col.begin() + A.ptr[r + 1], 0);
            A.val.insert(A.val.begin() + A.ptr[r + 1], 1.0);
            for (int64_t i = r + 1; i <= A.nrow; ++i) ++A.ptr[i];
            bool thrown = false;
            try {
                plan_coarse_rhs(c->P->mc, c->T);
            } catch (const ApiError& e) {
                thrown = e.code == DDPCA_EINVAL;
            }
            A = keep;
            acheck(thrown, "refusals: an entry of a subdomain that is not on the row's interface graph");
        }
        bool thrown = false, fits = w32(INT32_MAX) == INT32_MAX && w32(0) == 0;
        try {
            w32((int64_t)1 << 31);
        } catch (const ApiError& e) {
            thrown = e.code == DDPCA_EINVAL;
        }
        acheck(thrown && fits, "refusals: a W index of 2^31 does not narrow to int32");
        Rows rows(1);
        rows[0].push_back({(int64_t)1 << 31, 1.0});
        thrown = false;
        try {
            sell_pack(rows);
        } catch (const ApiError& e) {
            thrown = e.code == DDPCA_EINVAL;
        }
        acheck(thrown, "refusals: sell_pack refuses a column of 2^31");
        std::vector<std::pair<int32_t, double>> row = {{5, 1.0}, {2, 0.5}, {5, 2.0}, {2, 0.25}, {7, -1.0}};
        sum_duplicates(row);
        acheck(row == std::vector<std::pair<int32_t, double>>({{2, 0.75}, {5, 3.0}, {7, -1.0}}), "sum_duplicates sorts by column and sums in input order");
        const Csr M = triplets_to_csr({1, 0, 2.0, 0, 1, 1.0, 1, 0, 3.0}, 3, 2);
        acheck(M.ptr == std::vector<int64_t>({0, 1, 2}) && M.col == std::vector<int32_t>({1, 0}) && M.val == std::vector<double>({1.0, 5.0}),
               "triplets_to_csr sums duplicate entries");
        acheck(count_distinct(std::vector<int32_t>{3, 1, 3, 2, 1}) == 3, "count_distinct");
        std::printf("{\"case\": \"admm_plan_refusals\"}\n");
    }
}

// the refined octree as the one subdomain of a problem with an interface-eliminated coarse space on
// level 1: a hanging level (nh > 0) and rotated nodes (the CSR rows of the factored prolongation)
void admm_plan_octree(ddpca_multigrid_t g) {
    AdmmCase c;
    ok(ddpca_problem_empty(1, 0, &c.p), "problem_empty");
    if (!c.p) return;
    // the tree-built grid itself (as ESTABLISH leaves a generator's: MULTISCALE_1 composes its stencils)
    c.P = reinterpret_cast<Problem*>(c.p);
    c.owner = {0};
    MCONTACT& mc = c.P->mc;
    bool built = false;
    mc.multGrid[0] = *multigrid_of(g, &built);
    if (mc.multGrid[0].nodeAll) mc.multGrid[0].hangProl = mc.multGrid[0].hangRows();
    c.P->owned = {1};
    c.P->established = true;
    mc.muscSett = 2;
    mc.doleMcsc = {1};
    try {
        mc.MULTISCALE_1(nullptr);
        plan_case_tables(c, AdmmTuning(), "octree");
        acheck(c.T.subs.size() == 1 && c.T.subs[0].nh > 0 && c.T.NH >= c.T.subs[0].nh, "octree: a hanging level");
        plan_case_operators(c, "octree");
        plan_case_coarse(c, "octree", true);
    } catch (const std::exception& e) {
        acheck(false, std::string("octree: ") + e.what());
    }
}

}  // namespace

int main(int argc, char** argv) {
    std::setvbuf(stdout, nullptr, _IONBF, 0);  // the case lines before any sanitizer report
    const bool quick = argc > 1 && std::strcmp(argv[1], "quick") == 0;
    std::vector<Case> cases = {
        {"beam", {8, 2, 2, 1, 1, 1, 1}, 0, 1},        // beam_s1
        {"beam", {8, 2, 2, 2, 1, 1, 1}, 0, 1},        // beam_s2
        {"beam", {8, 2, 2, 1, 2, 1, 1}, 0, 1},        // beam_dd
        {"beam", {4, 2, 2, 2, 2, 1, 1}, 2, 1},        // beam_dd_m2
        {"beam", {4, 2, 2, 2, 2, 1, 1}, 2, 2},        // ... rank-local on 2 ranks
        {"twoblock", {0.0, 2}, 0, 1},                 // twoblock_f0
        {"twoblock", {0.3, 2}, 0, 1},                 // twoblock_f3
        {"twoblock", {0.0, 2}, 2, 1},                 // twoblock_f0_m2
        {"twoblock", {0.3, 2}, 1, 1},                 // twoblock_f3_m1
        {"twoblock", {0.3, 2}, 1, 2},                 // ... rank-local on 2 ranks
        {"dehw", {2, 2, 2, 1, 2, 0.3}, 2, 1},         // the synthetic chain, 4 subdomains
        {"dehw", {2, 2, 2, 1, 2, 0.3}, 2, 4},         // ... one subdomain per rank
        {"dehw", {2, 2, 2, 1, 2, 0.3}, 1, 2},         // LATIN coarse space, 2 ranks
        {"dehw", {4, 3, 2, 2, 2, 0.2, 2, 1}, 2, 1},   // the headline workload's shape at gl 2
    };
    if (quick) cases.resize(3);
    for (const auto& c : cases) run_case(c);
    // refused generator arguments
    {
        ddpca_problem_t p = nullptr;
        const double bad[7] = {7, 2, 2, 1, 2, 1, 1};
        refused(ddpca_problem_create("beam", bad, 7, &p), "beam 7 elements on 2 subdomains");
        refused(ddpca_problem_create("beam", bad, 3, &p), "beam 3 params");
        refused(ddpca_problem_create("no_such_kind", bad, 7, &p), "unknown kind");
    }
    run_octree();
    run_csearch();
    run_writers();
    run_mass_plan();
    run_mgpis_plan();
    run_admm_plan();
    std::printf("{\"ok\": %s, \"failures\": %d}\n", g_fail ? "false" : "true", g_fail);
    return g_fail ? 1 : 0;
}
