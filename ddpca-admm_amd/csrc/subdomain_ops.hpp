// The device solver's view of one established subdomain: the one place that decides which of the
// host grid's operators a MgpisDevice member is built from (ddpca_problem_mgpis,
// ddpca_problem_mgpis_batch and the MCONTACT batch all take it from here).
#pragma once
#include "mgpis_plan.hpp"
#include "multigrid.hpp"

namespace ddpca {

// The pointers reference g: it must outlive the MgpisDevice constructor call.
inline SubdomainOps subdomain_ops(const MULTIGRID& g) {
    SubdomainOps o;
    o.nnodes.assign(g.leveCount.begin(), g.leveCount.end());
    for (const auto& b : g.levelStif) o.K.push_back(&b);
    // prolOper: scalProl with the nodal rotations' 3x3 blocks as block entries (MULTIGRID.h:
    // 1141-1181; == scalProl without nodeRota), which the Galerkin operators are built with; an
    // operator-level subdomain has scalProl only (its block entries already in it)
    for (const auto& s : g.prolOper.empty() ? g.scalProl : g.prolOper) o.S.push_back(&s);
    o.dof_free = g.consFlag.data();
    o.coords = g.nodeCoor.empty() ? nullptr : g.nodeCoor[0].data();
    return o;
}

}  // namespace ddpca
