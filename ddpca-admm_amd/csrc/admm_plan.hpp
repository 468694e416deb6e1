// Host-side setup of the ADMM handle (device_mcontact.hip): everything that is derived from the
// established problem before it reaches the device -- the workspace layout W = [u | u_h | aux,
// lambda | gamma], the side and interface tables, the factored per-ip operands, the row lists of
// the SELL-64 interface operators and their packing, the coupling rows of the body-balance
// right-hand side, the hanging-level rows, the coarse right-hand side's per-source slots, the
// dense / DOUBLE_M decision with the DOUBLE_M hierarchy, the prolongation tables, and the byte
// models.  Plain C++ (no HIP), so the host sanitizer build covers it (tests/sanitize).  The vectors
// of a plan correspond one to one to the DevBuf members of the handle, which shares the plans'
// scalar parts as base classes; build() and build_coarse() upload a plan and drop it before the
// next one exists.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "../../include/ddpca_amd.h"
#include "mcontact.hpp"
#include "problem.hpp"
#include "sparse.hpp"

namespace ddpca {

// Create-time tuning variables, read once per create (admm_tuning); the plan functions take the
// struct and read no environment.
struct AdmmTuning {
    bool mass_fused = true;           // DDPCA_MASS_FUSED=0: the sequential aux / lambda update (A/B, tests)
    int64_t coarse_mg_min = 120000;   // DDPCA_COARSE_MG_MIN: rows from which DOUBLE_M(_1) solves the coarse problem (DIRE_MAXI, PREP.h:69)
    double coarse_dense_mb = 1024.0;  // DDPCA_COARSE_DENSE_MB: the dense inverse's budget per rank, MiB
    int64_t pcg_maxit = 0;            // DDPCA_PCG_MAXIT (diagnostics only): cap of the body solves, 0 = the reference's maxit = rows
    bool verbose = false;             // DDPCA_VERBOSE: the create path's lines on stderr
};
AdmmTuning admm_tuning();

// A workspace index as the int32 the kernels read: DDPCA_EINVAL past 2^31 - 1 (or below 0), never
// a wrapped index.
int32_t w32(int64_t w);

// distinct values of v (the byte models count every gathered entry once)
template <typename T>
int64_t count_distinct(std::vector<T> v) {
    std::sort(v.begin(), v.end());
    return (int64_t)(std::unique(v.begin(), v.end()) - v.begin());
}

// a row's entries stably sorted by column, duplicates summed in that order
void sum_duplicates(std::vector<std::pair<int32_t, double>>& row);
// n x n CSR of ntrip (row, col, value) triplets stored as doubles, duplicates summed in input order
Csr triplets_to_csr(const std::vector<double>& trip, int64_t ntrip, int64_t n);

// ---- what the plan sees of the owned subdomains' batch (MgpisDevice's host-side data; the same
// from mgpis_numbering and the LevelShape / TransferShape parts of plan_level / plan_transfer).
// Empty without an owned subdomain.
struct BatchLevelView {
    int64_t nn = 0;                            // padded nodes of the batch's level
    std::vector<int64_t> noff, nloc, tent_sub;  // per member: first node, real nodes, scalar transfer entries
    bool lat = false;                          // lattice transfer from the level below
};
struct BatchView {
    std::vector<BatchLevelView> lev;
    const std::vector<std::vector<std::vector<int32_t>>>* level_perm = nullptr;  // [l][s][reference local node] = device local node
    std::vector<int64_t> nfree;                // per member: free dofs of the fine level
    bool empty() const { return lev.empty(); }
    const std::vector<int32_t>& fine_perm(int s) const { return (*level_perm)[lev.size() - 1][s]; }
    int64_t fine_dof_offset(int s) const { return 3 * lev.back().noff[s]; }
    int64_t fine_dof(int s, int64_t dof) const { return 3 * (lev.back().noff[s] + fine_perm(s)[dof / 3]) + dof % 3; }
};

// ---- SELL-64 over W: row lists -> chunks of 64 rows, slot-major (rows padded to a multiple of
// 64; padding slots: column 0, value 0)
using Rows = std::vector<std::vector<std::pair<int64_t, double>>>;
struct SellShape {
    int64_t nrow = 0, nch = 0;
    // algorithmic bytes of one apply: the stored entries (8 B value + 4 B column), each distinct
    // gathered W entry once, every real row written once (an `add` operand adds 8 B per row)
    double bytes = 0.0;
};
struct SellPlan : SellShape {
    std::vector<int32_t> slots, col;
    std::vector<int64_t> off;
    std::vector<double> val;
};
SellPlan sell_pack(const Rows& rows);

// ---- tables
// workspace W = [u (NU) | u on hanging levels (NH) | aux, lambda (2R) | gamma (G)] and its regions
struct AdmmLayout {
    int64_t nsub = 0, nint = 0;
    int64_t R = 0;  // padded rows of all owned sides
    int64_t NU = 0, NH = 0, G = 0, oH = 0, oS = 0, oG = 0;
};
struct AdmmSub {
    int64_t tv = 0, nn = 0;
    int64_t dof0 = 0;  // first dof in the batch's fine layout
    int64_t nh = 0;    // hanging-level dofs (MULTIGRID::hangProl rows), at W[oH + hoff]
    int64_t hoff = 0;
    // workspace index of the subdomain's nodal dof c (position numbering, hanging level last)
    int64_t wcol(int64_t c, int64_t oH) const { return c < 3 * nn ? dof0 + c : oH + hoff + (c - 3 * nn); }
};
struct AdmmSide {
    int64_t ts = 0, s = 0, tv = 0, m = 0, mip = 0;
    int64_t roff = 0;  // rows of aux at W[oS + roff], lambda at W[oS + R + roff]
    int sub = 0;       // index into subs
};
struct AdmmItf {
    int64_t ts = 0, mip = 0, goff = 0;
    int comp = 1;
    double fric = -1.0;
    int owner[2] = {0, 0};
    bool mine = false, cross = false;
};
// the owned subdomains (tv, nn, nh), in batch order: what the batch's operators are taken from;
// DDPCA_ESTATE when one of them was not established on this rank
std::vector<AdmmSub> owned_subdomains(const Problem& P, const std::vector<int32_t>& owner, int rank);

struct AdmmTables : AdmmLayout {
    std::vector<AdmmSub> subs;
    std::vector<AdmmSide> sides;
    std::vector<AdmmItf> itfs;                                // by ts; gamma: cross-rank interfaces first, then rank-local
    std::map<std::pair<int64_t, int64_t>, size_t> side_of;    // (ts, s) -> owned side
    std::vector<int64_t> maxit;                               // per owned subdomain: n_free (reference maxit = rows)
    std::vector<double> cf;                                   // consForc, solver (device) node order
    std::vector<double> presc;                                // Dirichlet values, reference node order (3 nn_L)
    std::vector<int32_t> onode;                               // device node -> reference-order node of the batch
    const AdmmItf& itf_of(int64_t ts) const { return itfs[ts]; }
};
AdmmTables plan_tables(const MCONTACT& mc, std::vector<AdmmSub> subs, const std::vector<int32_t>& owner, int rank,
                       const BatchView& V, const AdmmTuning& tune);

// ---- interfaces whose per-ip operators are applied in factored form (Interface::factored)
struct FactItfShape {
    int64_t ts = 0, nip = 0, goff = 0;
    int C = 1, own[2] = {0, 0};
    double pen[3] = {0.0, 0.0, 0.0};
    int64_t nnc[2] = {0, 0}, roff[2] = {0, 0};   // node-major inteInpo (fused update)
    double bytes_gamma = 0.0, bytes_inpo = 0.0;  // algorithmic bytes of k_gamma_ip / k_traction_ip + k_inpo_node
};
struct FactItfPlan : FactItfShape {
    std::vector<double> B, M[2];
    std::vector<int32_t> lam[2], u[2];
    std::vector<int64_t> nptr[2];
    std::vector<int32_t> niq[2];
    std::vector<double> ncoef[2];
};
FactItfPlan plan_factored(const MCONTACT& mc, const AdmmTables& T, const AdmmItf& I);

// ---- interface operators over W (MCONTACT.h:2632-2636, 2671-2704)
// fused update: every owned side has inteMass_pena = rho inteMass and systTran_pena = rho systTran
// with rho = penN = penF (entries agree to rounding), and the tuning allows it
bool fused_update(const MCONTACT& mc, const AdmmTables& T, const AdmmTuning& tune);
struct AdmmOperators {
    SellPlan gamma, gamma1, aux, lam;  // gamma (my halves), rank-local interfaces' side-1 halves, aux RHS, lambda RHS
    bool has_gamma1 = false;
    std::vector<int32_t> gam1_dst;
    std::vector<double> gcst;
};
// (the fused update applies op_wv instead of op_aux / op_lam: their rows are built only for the
// sequential update)
AdmmOperators plan_operators(const MCONTACT& mc, const AdmmTables& T, bool fused);
struct AdmmFused {
    SellPlan wv;
    std::vector<double> rinv;
};
AdmmFused plan_fused(const MCONTACT& mc, const AdmmTables& T);
// the systems of a surface-mass batch: 0 inteMass_pena (aux), 1 inteMass (lambda), 2 inteMass twice
// ([w | v], the fused update)
struct MassList {
    std::vector<const Csr*> A;
    std::vector<int64_t> roff;
    int64_t nrow = 0;
};
MassList mass_list(const MCONTACT& mc, const AdmmTables& T, int which);

// ---- coupling rows of the body-balance RHS: sum over incident sides of
//      [systTran_pena | -systTran] on free dofs, solver dofs x W columns
struct CouplingPlan {
    std::vector<int32_t> crow;  // solver dofs, surface rows only
    std::vector<int64_t> cptr;
    std::vector<int32_t> ccol;  // columns index W
    std::vector<double> cval;
    double bytes = 0.0;         // k_cpl
};
CouplingPlan plan_coupling(const MCONTACT& mc, const AdmmTables& T, const BatchView& V);
// hanging-level values over u: one SELL-64 product (rows of prolOper[maxiLeve])
SellPlan plan_hanging(const MCONTACT& mc, const AdmmTables& T);

// per-ADMM-iteration byte model of the launches outside the PCG, mass CG and coarse space
struct AdmmBytes {
    double rhs = 0.0, iface = 0.0, moni = 0.0;
};
AdmmBytes admm_byte_model(const AdmmTables& T, bool fused, double coupling_bytes, const SellShape& hang, const SellShape& gamma,
                          const SellShape& gamma1, int64_t ngam1, const std::vector<const FactItfShape*>& fact,
                          const SellShape& aux, const SellShape& lam, const SellShape& wv);

// ---- coarse space
// the coarse right-hand side's per-source slots: sptr the slots of each coarse row, srcs their
// source subdomains in ascending order -- the same on every rank
struct CoarseSlots {
    std::vector<std::vector<int64_t>> srcs;
    std::vector<int64_t> sptr;
    // DDPCA_EINVAL when subdomain tv is not on row r's interface graph
    int64_t slot_of(int64_t r, int64_t tv) const;
};
struct CoarseRhsPlan {
    std::vector<int64_t> own_rows;  // global coarse rows of this rank, in xc order
    std::vector<int64_t> xoff;      // per owned subdomain: its first entry of xc
    CoarseSlots slots;
    int64_t nslot = 0;
    std::vector<int64_t> rptr;      // per slot: its entries over W, in a rank-independent order
    std::vector<int32_t> rcol;
    std::vector<double> rval;
    std::vector<double> f0;         // globForc_1 in the slot of the row's own subdomain
    double bytes = 0.0;
};
CoarseRhsPlan plan_coarse_rhs(const MCONTACT& mc, const AdmmTables& T);

struct CoarseSolveChoice {
    bool mg = false;         // DOUBLE_M(_1) instead of the dense inverse
    bool mg_gather = false;  // a rank-local build: the whole operator is gathered at coarse_invert
    double dense_bytes = 0.0;
    double bytes = 0.0;      // of the solve per correction (without DOUBLE_M's PCG)
};
CoarseSolveChoice coarse_solve_choice(const CoarseSpace& cs, int64_t nown, int nranks, const AdmmTuning& tune);
// this rank's rows of globCoup_1, dense n x n (zeros elsewhere)
std::vector<double> coarse_dense_rows(const CoarseSpace& cs, const std::vector<int64_t>& own_rows, int rank);

// the coarse MGPIS's structure: nodes per level, transfers, the coarse rows' dofs, per-level dof
// flags; kept until the operator is there (finish_coarse_mg)
struct MgPlan {
    std::vector<int64_t> nglob;
    std::vector<Stencil> S;
    std::vector<int32_t> fdg;
    std::vector<std::vector<uint8_t>> flev;
    bool latin = false;
};
MgPlan plan_coarse_mg(const MCONTACT& mc, int64_t n);

// u += accuProl x_c.  Assembled (the caller's accuProl): CSR rows over the owned fine free dofs and
// the constrained dofs; factored: the scalar stencil (<= 8 parents) for every node it can hold,
// CSR rows (same arrays) for the rest -- nodes whose chain meets a nodal rotation's 3x3 block
struct CoarseProlongShape {
    int64_t npr = 0, ncd = 0, nxn = 0, qnn = 0;
    int dmin = 0;
};
struct KGroupPlan {  // stiffness part: level-d device values gathered into the owned coarse rows' own slots
    int level = 0;
    std::vector<int32_t> rows;
    std::vector<int64_t> src;
};
struct CoarseProlongPlan : CoarseProlongShape {
    std::vector<int64_t> pptr;
    std::vector<int32_t> pcol, ptgt, cdof;
    std::vector<double> pval;
    // factored only
    std::vector<KGroupPlan> kg;
    std::vector<int32_t> xsrc, qcol;
    std::vector<double> qw;
    std::vector<uint8_t> flag;
    double bytes_csr = 0.0, bytes = 0.0;  // the CSR rows' share, then the rest (added in this order)
};
CoarseProlongPlan plan_prolong_assembled(const MCONTACT& mc, const AdmmTables& T, const std::vector<int64_t>& xoff);
CoarseProlongPlan plan_prolong_factored(const MCONTACT& mc, const AdmmTables& T, const BatchView& V, const CoarseSlots& slots,
                                        const std::vector<int64_t>& xoff);

}  // namespace ddpca
