// Host-side setup of MgpisDevice (device_mgpis.hpp): everything that is derived from the members'
// operators before it reaches the device -- the device numbering, the SELL-BSR3 packing of a level
// with its smoother inverses, 16-bit columns and table, the reduced-precision value records, the
// transfer lists / lattice codes / block CSRs, the fine level's colour chunks with their byte
// model, and the dense coarse matrices.  Plain C++ (no HIP), so the host sanitizer build covers it
// (tests/sanitize).  The vectors of a plan correspond one to one to the DevBuf members of LevelDev
// and GsFine, which share the plans' scalar parts as base classes; the constructor uploads a plan
// and drops it before the next one exists.
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/ddpca_amd.h"
#include "mgpis_layout.hpp"
#include "sparse.hpp"

namespace ddpca {

// Create-time tuning variables, read once per create (mgpis_tuning); the plan functions take the
// struct and read no environment.
struct MgpisTuning {
    bool col16 = true;     // DDPCA_COL16=0: no 16-bit column offsets
    int h16_levels = 3;    // DDPCA_H16_LEVELS: the finest levels in block-exponent fp16 (+2 % over 1 under block
                           // Jacobi, profiles/r01_sweep_h16.txt; with the multicolour fine level 3 over 2 +1.1 % at 8
                           // subdomains, +0.4 % at 2, 1 over 2 -4 %, the same 18.0 PCG iterations, profiles/r04j/ab_h16.txt)
    int q8_levels = 64;    // DDPCA_Q8_LEVELS: precond_fp32 = 3 keeps the finest of those levels in int8 (default all)
    bool gs_band = true;   // DDPCA_GS_BAND=0: the colour sweeps cover every row
    bool lattice = true;   // DDPCA_LATTICE=0: explicit transfer lists only
    bool gs_r32 = true;    // DDPCA_GS_R32=0: the colour sweeps' residual stays fp64 (A/B)
    bool bj_x4 = true;     // DDPCA_BJ_X4=0: the block-Jacobi levels' iterates stay fp64 (A/B)
    bool verbose = false;  // DDPCA_VERBOSE: the create path's lines on stderr
};
MgpisTuning mgpis_tuning();

// Operators of one subdomain, in the host (MULTIGRID restatement) layout.
struct SubdomainOps {
    std::vector<int64_t> nnodes;           // nodes of level <= l
    std::vector<const Bsr3*> K;            // unconstrained Galerkin operator per level
    const uint8_t* dof_free = nullptr;     // 3 * nnodes.back() flags (consFlag)
    // optional per-level flags (3 * nnodes[l] each) where a dof's status differs between levels
    // (LATIN's DOUBLE_M: a coarse contact node its finer level does not carry is a masked copy
    // there); empty = the fine flags' prefix on every level (consOper, MULTIGRID.h:1186-1243)
    std::vector<const uint8_t*> dof_free_lev;
    const uint8_t* free_flags(int l) const { return dof_free_lev.empty() ? dof_free : dof_free_lev[l]; }
    std::vector<const Stencil*> S;         // scalar prolongation stencils, nlev - 1
    const double* coords = nullptr;        // optional 3 * nnodes.back() node coordinates: when
                                           // given, levels >= 1 are renumbered on the device
};

// ---- numbering
// Quantised (z, y, x) keys of a level's nodes: coordinates quantised to 1e-9 of the bounding
// box, so nodes of one mesh plane share a key despite rounding in their coordinates.
using Key3 = std::array<int64_t, 3>;
std::vector<Key3> quantised_keys(const double* xyz, int64_t n);
// Bit-exact row types of one level of one subdomain: masked block values in canonical slot order.
std::vector<int32_t> row_types(const Bsr3& A, const uint8_t* fr, const std::vector<Key3>& key, int64_t& ntypes);
// Device node order of one level, p[reference node] = device node: lexicographic in (z, y, x);
// with row types, grouped by type first (lexicographic inside a type), so 64-row chunks are
// type-homogeneous wherever a type has enough rows.
std::vector<int32_t> device_order(const std::vector<Key3>& key, const std::vector<int32_t>* type);
std::vector<int32_t> identity_order(int64_t n);

// perm[l][s][reference local node] = device local node.  Levels >= 1 with coordinates:
// lexicographic, or -- table mode, when the level's distinct rows compress -- grouped by row type
// so chunks are type-homogeneous; their slots go in canonical order (keys non-empty).
struct MgpisNumbering {
    std::vector<std::vector<std::vector<int32_t>>> perm;
    std::vector<std::vector<std::vector<Key3>>> keys;
    std::vector<char> grouped;
};
MgpisNumbering mgpis_numbering(const std::vector<SubdomainOps>& subs, int table_mode);

// ---- one level's operator
struct LevelShape {
    int64_t nn = 0, nch = 0, nslots = 0, nnzb = 0;  // batch totals (nn, nch padded)
    std::vector<int64_t> noff, nloc, nnzb_sub;      // per subdomain: first node, real nodes, blocks
    // table mode: rows whose block values (in device slot order, masks applied) are bit-identical
    // share one table row; the kernel streams only column indices and a row type, the values
    // come from the cache-resident table (structured meshes: ~30x fewer distinct rows than rows)
    bool tbl = false;
    int64_t tstride = 0;   // doubles per table row (max row length * 9)
    int64_t ntypes = 0;
    int64_t nuniform = 0;  // chunks whose rows all share one type
};

struct LevelPlan : LevelShape {
    std::vector<int32_t> slots, csub, col;  // per chunk: slots, subdomain; per slot lane: batch device column
    std::vector<int64_t> off;
    std::vector<int16_t> col16;  // col - row node when wanted and every offset fits, else empty
    bool fits16 = false;         // col16 was filled (the constructor drops the vector once it is uploaded)
    std::vector<double> val;     // masked blocks, val[(q * 9 + ij) * 64 + lane]: identity on constrained dofs,
                                 // pad rows and pad slots a self column with zero values
    std::vector<double> dinv, minv;  // point inverse (3 per node); the smoother's: 3, or 9 under block Jacobi
    std::vector<uint8_t> mask;       // bit a set = dof 3i+a free
    std::vector<int32_t> rtype, ctype;  // table mode
    std::vector<double> tab;
};
// bj: block-Jacobi inverses; table_mode as the option (levels >= 1 only)
LevelPlan plan_level(const std::vector<SubdomainOps>& subs, const MgpisNumbering& num, int l, bool bj, int table_mode,
                     const MgpisTuning& tune);

// the smoother inverse in fp32 for a reduced-precision level, symmetrised before rounding (block
// Jacobi, symmetric operators) so the V-cycle stays exactly symmetric
std::vector<float> smoother_inverse_fp32(const std::vector<double>& minv, bool bj, bool symmetrise);

// ---- value records: nslot slots of 64 blocks in one storage type (mgpis_layout.hpp)
struct BlockValues {
    int vt = kVal64;
    size_t n = 0;        // elements of the one array in use
    bool ok = true;      // false: an int8 scale left fp32's normal range (put)
    std::vector<uint8_t> v8;
    std::vector<uint16_t> v16;
    std::vector<float> v32;
    std::unique_ptr<double[]> v64;  // (not a vector: the fine level's copy is written in full, never zero-filled)
    // sparse: zero-filled and never empty (colour chunks: pad slots stay zero blocks); otherwise the
    // caller writes every block
    BlockValues(int vt, int64_t nslot, bool sparse);
    // the record of one block (9 fp64 entries at blk[0], blk[stride], ...) into (slot, lane)
    void put(int64_t slot, int64_t lane, const double* blk, int64_t stride);
};
// all of a level's blocks, in its slot order
BlockValues pack_values(const LevelPlan& P, int vt);
// the V-cycle copy of level l of nlev under precond_fp32 (>= 1): int8 or block-exponent fp16 on
// the finest levels the tuning names, fp32 below; a level with a block outside the int8 record's
// range -- entries beyond fp32's 3.4e38 or below ~1e-36 -- takes the fp16 copy, whose
// exponent has no such limit
int level_copy_type(int precond_fp32, int l, int nlev, const MgpisTuning& tune);
BlockValues level_copy(const LevelPlan& P, int vt, int l, const MgpisTuning& tune);

// ---- transfer from level l - 1 (batch-global indices)
struct TransferShape {
    std::vector<int64_t> tent_sub, tblk_sub;  // per subdomain: scalar stencil entries, 3x3 block entries
    bool uw = false;       // uniform averaging: prolongation weight = 1 / parent count (nested
                           // refinement), computed in k_prolong instead of read
    bool lat = false;      // lattice transfers (see TransferPlan)
    // block transfer entries (nodal rotations, MULTIGRID.h:1141-1181): P = S (x) I3 + sum of
    // 3x3 blocks, as CSR over the fine nodes that own one (prolongation) and over the coarse
    // nodes that receive one (restriction, B^T); nrot = 0 on plain S (x) I3 transfers
    int64_t nrot = 0, nrotc = 0;
};

struct TransferPlan : TransferShape {
    std::vector<int32_t> ppar;  // 8 x nn, slot-major, -1 = unused
    std::vector<double> pw;     // weights (unread when uw)
    // restriction: SELL-64 over the coarse nodes of level l-1 (chunk = 64 coarse nodes, lane =
    // node, slot k = k-th child: own fine copy first, padding = weight 0)
    std::vector<int32_t> rslots, rcol;
    std::vector<int64_t> roff;
    std::vector<double> rwt;
    // lattice transfers (uniform averaging on a lexicographically numbered box lattice, detected
    // at create): a fine node's parents are p0 + subset sums of three coarse strides, a coarse
    // node's children its fine copy f0 + sum d_k t_k (d in {-1,0,1}^3) with weight 2^-|d|
    std::vector<uint32_t> ppk, rmsk;   // per fine node: p0 | (stride-subset code << 29); per coarse node: children present, bit (d0+1) + 3(d1+1) + 9(d2+1)
    std::vector<int32_t> pstr, rstr, rf0;  // per subdomain: 3 coarse / fine strides; per coarse node: its fine copy
    // block entries, parents past the eighth as w*I blocks among them
    std::vector<int32_t> rot_row, rot_par, rotc_row, rotc_kid;
    std::vector<int64_t> rot_ptr, rotc_ptr;
    std::vector<double> rot_blk, rotc_blk;
};
// F, C: the shapes of levels l and l - 1; the lists stay filled when the lattice form is taken
TransferPlan plan_transfer(const std::vector<SubdomainOps>& subs, const MgpisNumbering& num, int l, const LevelShape& F,
                           const LevelShape& C, const MgpisTuning& tune);

// ---- multicolour Gauss-Seidel on the fine level
struct ColourShape {
    int ncol = 0;                        // colours
    int64_t nchunk = 0;                  // colour chunks of the batch, member-major, colour-minor
    std::vector<int64_t> first, count;   // per colour: its chunk ids in `list`
    std::vector<int64_t> nnzb_sub;       // per member: stored off-diagonal blocks (byte model)
    std::vector<int64_t> slots_sub;      // per member: L + U slots incl. padding
    // algorithmic bytes of each launch over the whole batch, in launch order: forward colours
    // 0..K-1, the residual, backward colours K-1..0 (stored blocks, per-row vectors, every distinct
    // x entry gathered once; profiles/gs_table.py sets the rocprof / PMC figures beside them)
    std::vector<double> launch_bytes;
    std::vector<double> gx_f, gx_b, rows_k;  // per colour: distinct x gathered (forward, backward), rows
    double gx_r = 0.0;                       // distinct x the residual gathers
    std::vector<double> gx_u, nl_k, nu_k;    // per colour: distinct U-side x gathered, L / U blocks
    double gx_l = 0.0, vb = 0.0;             // distinct L-side x over all colours; bytes per stored block
    double rowf = 0.0;                       // bytes per row of a sweep: b, the inverse, x written, the row index
    // band mode (locally refined fine level): the colours cover only the band -- the
    // nodes the fine level adds to the next coarser one and their neighbours; two more chunk groups
    // per member follow the colours: the ring (non-band rows with a band neighbour: their band
    // columns only, for the residual) and the far rows (no blocks).  first / count then hold ncol + 2
    // groups; the sweeps run over the colours, k_gs_aux over the ring and far groups.
    bool band = false;
    std::vector<int64_t> band_rows_sub, ring_rows_sub, far_rows_sub, ring_nnzb_sub;
};

struct ColourPlan : ColourShape {
    std::vector<int32_t> list, rowidx, csub, nsl, nsu, col;
    std::vector<int64_t> offl, offu, cb;
    std::vector<int16_t> col16;
    BlockValues val{kVal64, 0, true};
    std::vector<float> minvc;  // the rows' fp32 3x3 inverses in chunk order, [chunk][ij][lane]
};
// The band of a locally refined fine level l: the nodes it adds to level l - 1 (reference positions
// past nnodes[l - 1]) and their neighbours, per device node; empty when that is no row or more than
// 60 % of the rows, or when the tuning switches the band off
std::vector<uint8_t> colour_band(const std::vector<SubdomainOps>& subs, const MgpisNumbering& num, int l, const LevelPlan& P,
                                 const MgpisTuning& tune);
// The colour structure of level P in storage type vt; minv32 (or null: fp64 sweeps) the level's
// fp32 block inverses; band (or null) from colour_band.  Throws DDPCA_EINVAL past 64 colours or
// when vt is int8 and a block's scale is out of range.
ColourPlan plan_colours(const LevelPlan& P, int vt, const std::vector<float>* minv32, const std::vector<uint8_t>* band,
                        const MgpisTuning& tune);
// launch_bytes from the plan's counts: smoother 3 in the order above, with the 16-B iterate (x4)
// and residual (r4) where the sweeps run on fp32 copies; smoother 4 in k_gs_ssor's launch order
void colour_byte_model(ColourShape& G, int smoother, bool x4, bool r4);

// ---- exact coarse solve
// clev: the option, or the highest level below the fine one whose inverses of all members fit in
// 256 MB with at most 12,288 rows each (a few-subdomain batch trades the coarse levels'
// latency-bound launches for one GEMV over a larger dense inverse); never the fine level of a
// hierarchy.  *n0max: the largest member's rows there.
int choose_coarse_level(const std::vector<SubdomainOps>& subs, int coarse_level_opt, int64_t* n0max);
// member S's masked operator on level clev, dense row-major in device order p; a constrained dof's
// decoupled row and column carry 1, or in the general path the largest free diagonal entry
std::vector<double> coarse_dense(const SubdomainOps& S, int clev, const std::vector<int32_t>& p, bool general);
// after the inverse: constrained rows and columns zeroed, rows appended to `packed` at a stride of
// 3 nc rounded up to 4 (returned); DDPCA_ESTATE when that passes the member's padded rows
int64_t coarse_pack(std::vector<double>& D, const SubdomainOps& S, int clev, const std::vector<int32_t>& p,
                    int64_t padded_nodes, std::vector<double>& packed);

// ---- small pieces
bool invert3(const double m[9], double r[9]);
// Chebyshev coefficients of sweep k on [lmax/30, lmax] of M K (k = 0: the 1/theta start)
void cheb_coef(double lmax, int k, double& c1, double& c2);
// [(sweep * nsub + sub) * 2 + {0,1}], sweeps 0..nu: Chebyshev (c1, c2) / Jacobi (-, omega)
std::vector<double> smoother_coefs(const std::vector<double>& lmax, int nu, int smoother, double omega);
// batch fine-level dofs of member S's free dofs (p: its fine device order, noff: its first node)
std::vector<int32_t> free_dof_map(const SubdomainOps& S, const std::vector<int32_t>& p, int64_t noff);

}  // namespace ddpca
