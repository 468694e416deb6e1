// C ABI of the contact search with a chosen path (CSEARCH::BUCKET_SORT / CONTACT_SEARCH /
// SEGMENT_INTERSECT, CSEARCH.h:205-230, 614-817, and the selection of ADAPTIVE_REFINE,
// CSEARCH.h:839-956): ddpca_contact_search_on / ddpca_refine_select_on (device >= 0: the kernels of
// device_csearch.hip; -1: the host entries of csearch.cpp, unchanged; -2: the device path's own
// steps on the host) and the measurement getters.
#include <chrono>
#include <memory>

#include "../../include/ddpca_amd.h"
#include "device_common.hpp"
#include "device_csearch.hpp"

using namespace ddpca;

namespace {

// of the calling thread's last two-pass search (device >= 0 or -2): plan, upload, k_cs_count + scan,
// k_cs_emit, copy back; candidate pairs, kept pairs, points
thread_local double last_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
thread_local int64_t last_pairs[3] = {0, 0, 0};

void two_pass(int device, const CsearchInput& in, bool values, ddpca_ips& out) {
    if (device == -2) {
        csearch_two_pass_host(in, values, out, last_ms, last_pairs);
        return;
    }
    if (device < 0) throw ApiError(DDPCA_EINVAL, "contact search: device is an index >= 0, -1 (host) or -2 (two-pass host)");
    select_device(device);
    const auto t0 = std::chrono::steady_clock::now();
    const CsearchPlan P = csearch_plan(in);  // refuses what a bounded kernel cannot take, before any launch
    last_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    csearch_device(in, P, values, out, last_ms + 1, last_pairs);
}

}  // namespace

extern "C" {

int ddpca_contact_search_on(int device, const double* mast_xyz, int64_t mast_nnode, const double* slav_xyz,
                            int64_t slav_nnode, int64_t nm, const int64_t* mast_segm, const double* mast_2d, int64_t ns,
                            const int64_t* slav_segm, const double* slav_2d, const int64_t* buck, double maxiDist,
                            ddpca_ips_t* out) {
    if (device == -1)
        return ddpca_contact_search(mast_xyz, mast_nnode, slav_xyz, slav_nnode, nm, mast_segm, mast_2d, ns, slav_segm, slav_2d,
                                    buck, maxiDist, out);
    return guarded([&] {
        if (!out) throw ApiError(DDPCA_EINVAL, "null argument");
        const CsearchInput in{mast_xyz, mast_nnode, slav_xyz, slav_nnode, nm, mast_segm, mast_2d, ns, slav_segm, slav_2d, buck,
                              maxiDist};
        auto R = std::make_unique<ddpca_ips>();
        two_pass(device, in, true, *R);
        *out = R.release();
    });
}

int ddpca_refine_select_on(int device, const double* mast_xyz, int64_t mast_nnode, const double* slav_xyz, int64_t slav_nnode,
                           int64_t nm, const int64_t* mast_segm, const double* mast_2d, int64_t ns, const int64_t* slav_segm,
                           const double* slav_2d, const int64_t* buck, double distCrit, int64_t ne_m, const int64_t* mast_elem,
                           int64_t ne_s, const int64_t* slav_elem, uint8_t* mast_split, uint8_t* slav_split) {
    if (device == -1)
        return ddpca_refine_select(mast_xyz, mast_nnode, slav_xyz, slav_nnode, nm, mast_segm, mast_2d, ns, slav_segm, slav_2d,
                                   buck, distCrit, ne_m, mast_elem, ne_s, slav_elem, mast_split, slav_split);
    int any = 0;
    const int rc = guarded([&] {
        if ((ne_m > 0 && (!mast_elem || !mast_split)) || (ne_s > 0 && (!slav_elem || !slav_split)) || ne_m < 0 || ne_s < 0)
            throw ApiError(DDPCA_EINVAL, "null argument");
        const CsearchInput in{mast_xyz, mast_nnode, slav_xyz, slav_nnode, nm, mast_segm, mast_2d, ns, slav_segm, slav_2d, buck,
                              distCrit};
        ddpca_ips ips;
        two_pass(device, in, false, ips);  // the node ids of the kept pairs; no value array is made or copied
        any = refine_flags(ips, mast_nnode, slav_nnode, ne_m, mast_elem, ne_s, slav_elem, mast_split, slav_split);
    });
    return rc != 0 ? rc : any;
}

int ddpca_csearch_last_ms(double* out5) {
    return guarded([&] {
        if (!out5) throw ApiError(DDPCA_EINVAL, "ddpca_csearch_last_ms: null argument");
        for (int k = 0; k < 5; ++k) out5[k] = last_ms[k];
    });
}

int64_t ddpca_csearch_last_pairs(int64_t* out3) {
    return guarded([&] {
        if (!out3) throw ApiError(DDPCA_EINVAL, "ddpca_csearch_last_pairs: null argument");
        for (int k = 0; k < 3; ++k) out3[k] = last_pairs[k];
    });
}

}  // extern "C"
