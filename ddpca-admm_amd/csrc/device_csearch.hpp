// Two-pass contact search (CSEARCH::BUCKET_SORT / CONTACT_SEARCH / SEGMENT_INTERSECT,
// CSEARCH.h:205-230, 614-817, and the selection of ADAPTIVE_REFINE, 839-956): the plan the host
// builds (csearch.cpp), the result arrays, and the device entry (device_csearch.hip).  No HIP type
// in this header: csearch.cpp includes it too.
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/ddpca_amd.h"

// the integration points in ddpca_ips_get's layout: node[n][2][4], shap[n][2][4], basis[n][3][3],
// gap[n], w[n].  A search that was asked for the node ids only (ddpca_refine_select_on) leaves the
// value arrays empty (values = false).  Plain arrays, not vectors: every element is written by the
// search, and zero-filling 216 B per point first would cost as much as the copy back.
struct ddpca_ips {
    int64_t n = 0;
    bool values = false;
    std::unique_ptr<int64_t[]> node;
    std::unique_ptr<double[]> shap, basis, gap, w;
    void resize(int64_t count, bool with_values) {
        n = count;
        values = with_values;
        node.reset(new int64_t[(size_t)8 * count]);
        shap.reset(with_values ? new double[(size_t)8 * count] : nullptr);
        basis.reset(with_values ? new double[(size_t)9 * count] : nullptr);
        gap.reset(with_values ? new double[(size_t)count] : nullptr);
        w.reset(with_values ? new double[(size_t)count] : nullptr);
    }
};

namespace ddpca {

// the arguments of ddpca_contact_search
struct CsearchInput {
    const double* mast_xyz;
    int64_t mast_nnode;
    const double* slav_xyz;
    int64_t slav_nnode;
    int64_t nm;
    const int64_t* mast_segm;
    const double* mast_2d;
    int64_t ns;
    const int64_t* slav_segm;
    const double* slav_2d;
    const int64_t* buck;
    double maxiDist;
};

// What the host decides before any pair is evaluated.  The bucket CSR holds the masters of a bucket
// in insertion order (ascending index); the pair list is in the reference's order (slave face,
// bucket row, bucket column, position in the bucket); pair_off[t] .. pair_off[t + 1] are slave face
// t's pairs (none for a face outside the bucket range: cell[t] = -1).
struct CsearchPlan {
    std::vector<int64_t> bucket_ptr;
    std::vector<int32_t> bucket_face;
    std::vector<int64_t> cell;
    std::vector<int32_t> pair_slav, pair_mast;
    std::vector<int64_t> pair_off;
    std::vector<int32_t> mast_face, slav_face;  // the faces' node ids, 4 per face
    long cap = 1;  // trip cap of PROJECT_STM's stepped approach
};

constexpr long kCsearchMaxCap = 1L << 20;

// Checks the input as search() does and, beyond it, what a bounded kernel needs (finite
// coordinates, every master face's shortest corner distance > 0, a trip cap <= 2^20, fewer than
// 2^31 nodes and faces), then builds the plan with search()'s own expressions for the bucket grid.
// Throws ApiError(DDPCA_EINVAL).
CsearchPlan csearch_plan(const CsearchInput& in);

// The search on the host by the device path's own steps (device = -2): count per pair, exclusive
// scan, emit the kept pairs at their offsets; OpenMP over pairs, csearch_face.hpp arithmetic.
// values = false: node ids only.  pairs: candidate pairs, kept pairs, points.  ms: plan, 0, count +
// scan, emit, 0 (host clock).
void csearch_two_pass_host(const CsearchInput& in, bool values, ddpca_ips& out, double ms[5], int64_t pairs[3]);

// The same on `device` (current, selected by the caller): upload, k_cs_count, scan of the copied-back
// counts on the host, k_cs_emit, copy back.  Every buffer lives for the call only; a failed
// allocation throws ApiError(DDPCA_EHIP) naming what was being allocated and its size.  ms: upload,
// k_cs_count (HIP events) + copy of the counts + scan (host clock), k_cs_emit (HIP events), copy back.
void csearch_device(const CsearchInput& in, const CsearchPlan& plan, bool values, ddpca_ips& out, double ms[4],
                    int64_t pairs[3]);

// ddpca_refine_select's flagging from the node ids of the kept pairs' points; returns isnoRefi
int refine_flags(const ddpca_ips& ips, int64_t mast_nnode, int64_t slav_nnode, int64_t ne_m, const int64_t* mast_elem,
                 int64_t ne_s, const int64_t* slav_elem, uint8_t* mast_split, uint8_t* slav_split);

}  // namespace ddpca
