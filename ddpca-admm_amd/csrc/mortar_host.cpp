// The device path of the mortar operators, walked on the host (device = -2; mortar_plan.hpp): the
// plan, then the bodies of the kernels' threads (mortar_point.hpp) in the kernels' order -- one
// contact node after the other with its partners in passes of 64 lanes, one pair, one incidence-list
// position, one point at a time.  Everything but the launch runs here, and is sanitized, without a GPU.
#include <algorithm>

#include "mortar_plan.hpp"

namespace ddpca {

namespace {

template <int C>
void walk_side(mortar::MortarView& V) {
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t c = 0; c < V.ncn; ++c) {
        const int32_t np = V.pptr[c + 1] - V.pptr[c];
        for (int32_t t0 = 0; t0 < np; t0 += 64)  // the wavefront's passes
            for (int32_t t = t0; t < std::min(np, t0 + 64); ++t) mortar::pair_lane<C>(V, (int32_t)c, t);
    }
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < V.npair; ++k) mortar::nodal_emit<C>(V, k);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < V.ninc + V.nip; ++i) {
        if (i < V.ninc) mortar::inpo_emit<C>(V, i);
        else mortar::point_emit<C>(V, i - V.ninc);
    }
}

}  // namespace

void mortar_build_host(const MortarInput& in, Interface& itf) {
    MortarPlan P = mortar_plan(in);
    MortarValues val[2];
    for (int s = 0; s < 2; ++s) {
        const MortarSide& S = P.side[s];
        MortarValues& v = val[s];
        mortar::MortarView V = S.view(s, in.C, in.penN, in.penF);
        V.pts = reinterpret_cast<const double*>(in.ip);
        v.aGP.resize(9 * S.npair);
        if (in.C == 3) v.aG.resize(9 * S.npair);
        else v.aN.resize(3 * S.npair), v.aM.resize(S.npair);
        v.mass.resize(V.n_mass), v.tran.resize(V.n_tran), v.tranp.resize(V.n_tran);
        v.imass.resize(V.n_imass), v.imassp.resize(V.n_imass);
        v.lagr.resize(V.n_lagr), v.disp.resize(V.n_disp), v.pema.resize(V.n_disp), v.inpo.resize(V.n_inpo);
        V.aGP = v.aGP.data(), V.aG = v.aG.data(), V.aN = v.aN.data(), V.aM = v.aM.data();
        V.mass = v.mass.data(), V.tran = v.tran.data(), V.tranp = v.tranp.data();
        V.imass = v.imass.data(), V.imassp = v.imassp.data();
        V.lagr = v.lagr.data(), V.disp = v.disp.data(), V.pema = v.pema.data(), V.inpo = v.inpo.data();
        if (in.C == 3) walk_side<3>(V);
        else walk_side<1>(V);
    }
    mortar_finish(in, P, val, itf);
}

}  // namespace ddpca
