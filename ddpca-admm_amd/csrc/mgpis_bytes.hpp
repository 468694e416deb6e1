// Algorithmic byte model and launch count of MgpisDevice's solve path (every input
// read once, every output written once, a gathered vector counted once per element), per batch
// member.  It restates by hand the launch sequence that vcycle() and enqueue_iteration() issue, and
// it gives every roofline figure and the launch counts the benchmark reports.  Plain C++ (no HIP):
// it reads MgpisBytes, the counts and flags of a handle that the constructor records once the
// reduced-precision copies are settled, so the host sanitizer build covers it (tests/sanitize).
#pragma once
#include <cstdint>
#include <vector>

#include "mgpis_plan.hpp"

namespace ddpca {

struct MgpisBytes {
    // a level: its shapes (per member nloc, nnzb_sub, tent_sub, tblk_sub; tbl, ntypes, tstride, lat, uw)
    struct Level : LevelShape, TransferShape {
        int vt = kVal64;     // storage type of the V-cycle's copy (MgpisDevice::vc_type)
        bool col16 = false;  // 16-bit column offsets
        bool x4 = false;     // fp32 iterate copies (LevelDev::x4a)
    };
    // the fine level's colours (ncol = 0: none): the counts of ColourShape, band included
    struct Colours : ColourShape {
        int vt = kVal64;
        bool col16 = false;
        bool x4 = false, r4 = false;  // fp32 iterate / residual copies (GsFine::x4, r4)
    };
    std::vector<Level> lev;
    Colours gs;
    int nu = 1, smoother = 0;
    int clev = 0;         // the level of the dense coarse solve
    bool ainv32 = false;  // its inverses are stored in fp32
};

// Output pairs: [0] fine-level kernels (the transfers to and from the fine level included), [1]
// every launch below it and the scalar kernels.
// operator bytes of one fine pass, member s, values in storage type vt (prod_cols: with the 16-bit
// column offsets where the level has them)
double fine_matrix_bytes(const MgpisBytes& M, int s, int vt, bool prod_cols = true);
double fine_kernel_bytes(const MgpisBytes& M, int s);  // one fine-level k_sell<kPcg>
void vcycle_bytes(const MgpisBytes& M, int s, double out[2]);
void iteration_bytes(const MgpisBytes& M, int s, double out[2]);  // SpMV + axpy + V-cycle + scalars
void setup_bytes(const MgpisBytes& M, int s, double out[2]);      // x0 = 0 initialisation + the first V-cycle
// launches of one PCG iteration.  Known gaps: the extra launches of transfers with
// rotation block entries are not counted, and a colour launch over an empty group still is.
int64_t iteration_launches(const MgpisBytes& M);

}  // namespace ddpca
