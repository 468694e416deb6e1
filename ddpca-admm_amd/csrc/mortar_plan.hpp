// The plan of one interface's mortar operators (Interface::BUILD, mcontact.cpp: MCONTACT.h:181-810,
// CONT_ROTA 157-179): everything in BUILD that is an index and not a value, built on the host in
// plain C++ (mortar_plan.cpp), and the walk of the device path's own steps on the host
// (mortar_host.cpp, device = -2).  No HIP type in this header: the CPU tests and the sanitizer
// driver reach it.  The values are the kernels' (device_mortar.hip) or the host walk's, both through
// mortar_point.hpp.
#pragma once
#include <cstdint>
#include <vector>

#include "mcontact.hpp"
#include "mortar_point.hpp"

namespace ddpca {

// What BUILD reads: the points, comp(), the penalties, and per side the node count and nodeRota.
struct MortarInput {
    const IntegralPoint* ip = nullptr;
    int64_t nip = 0;
    int C = 3;  // comp()
    double penN = 0.0, penF = 0.0;
    int64_t nn[2] = {0, 0};
    const NodeRota* rot[2] = {nullptr, nullptr};  // null: no rotation
};

// One side.  int32 throughout what the kernels index with: mortar_plan refuses what does not fit.
struct MortarSide {
    int64_t nn = 0, ncn = 0, nip = 0, npair = 0, ninc = 0;
    std::vector<int64_t> nodeCont;   // contact index -> body node id, insertion order
    std::vector<int32_t> ipc;        // 4 per point: the contact indices of its nodes
    // the incidence list: contact node c's entries 4 q + a at inc[inc_ptr[c] .. inc_ptr[c + 1]),
    // ascending (q, then a).  It is the summation order of the pair sums (q, a, then b) and the fill
    // order of inteInpo's rows: the entry of rank r lands at ptr[C c + k] + C r + m.
    std::vector<int32_t> inc_ptr, inc;
    std::vector<int32_t> inc_node;   // per list position: its contact node
    std::vector<int32_t> pptr, part; // sorted, unique partners
    std::vector<int32_t> pair_node;  // per pair: its contact node
    std::vector<int32_t> bypos;      // partners ordered by body node id (systMass), per pair position
    std::vector<int32_t> byrank;     // its inverse: pair pptr[a] + t sits at position byrank of a's systMass row
    std::vector<int32_t> nrow0;      // per contact node: the pairs of the contact nodes with a smaller body node id
    std::vector<uint8_t> ord_c, ord_n;  // 4 per point: the permutations of BUILD's two std::sorts
    std::vector<int32_t> rotidx;     // per contact node: index into rot, -1 for none
    std::vector<double> rot;         // 9 per rotated contact node, row-major
    bool rotated = false;            // a contact node of this side has a rotation
    // ptr and col of the nine operators as BUILD lays them out (val empty)
    Csr systMass, systTran, systTran_pena, inteMass, inteMass_pena, inpoLagr, inpoDisp, inteInpo, pemaInpo_r;
    // the view of mortar_point.hpp over these arrays (host pointers); points, sums and values unset
    mortar::MortarView view(int s, int C, double penN, double penF) const;
};

struct MortarPlan {
    int C = 3;
    bool factored = true;
    MortarSide side[2];
};

// count or offset -> int32, or DDPCA_EINVAL naming what does not fit
int32_t mortar_i32(int64_t v, const char* what);

// Builds the plan.  DDPCA_EINVAL: a node id outside [0, nn), a count or offset the int32 col arrays
// or the kernels' int32 indices cannot hold.
MortarPlan mortar_plan(const MortarInput& in);

// the storage of one side's pair sums and operator values, and the view pointed at it
struct MortarValues {
    std::vector<double> aGP, aG, aN, aM;
    std::vector<double> mass, tran, tranp, imass, imassp, lagr, disp, inpo, pema;
};

// Moves the plan's patterns and the values of both sides into the interface's members, with
// nodeCont, inpoNgap, pemaDiag and `factored` (the trivial parts, on the host).
void mortar_finish(const MortarInput& in, MortarPlan& plan, MortarValues (&val)[2], Interface& itf);

// The device path's own steps on the host (device = -2): the plan, then pair_lane / nodal_emit /
// inpo_emit / point_emit of mortar_point.hpp in the kernels' order, OpenMP over contact nodes, pairs,
// list positions and points.  Fills the same Interface members as BUILD.
void mortar_build_host(const MortarInput& in, Interface& itf);

// MortarInput of an interface's own points and parameters
MortarInput mortar_input(const Interface& itf, const int64_t nn[2], const NodeRota* const rot[2]);

}  // namespace ddpca
