// Device stress recovery (device_stress.hip): MULTIGRID::STRESS_RECOVERY, MULTIGRID.h:1316-1433.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ddpca_amd.h"
#include "multigrid.hpp"

namespace ddpca {

// Nodal stresses of g's tree on `device` (current, selected by the caller).  The displacement is
// device-resident, in positions, in two ranges as the MCONTACT workspace keeps it: the dofs of the
// nodes [0, nsplit) at u_main, those of [nsplit, nodalCount) at u_hang (one array: u_hang =
// u_main + 3 nsplit).  The plan is uploaded on the first call and kept with g (StressPlan::device).
// Enqueues on `stream` and returns the device result, 7 nodalCount doubles owned by the plan,
// valid until the next call on the same tree.
const double* stress_device(MULTIGRID& g, int device, const double* u_main, const double* u_hang, int64_t nsplit,
                            hipStream_t stream);

// HIP-event times of the last stress_device call on g, once its stream is synchronised:
// out[0] k_stress_elem, out[1] k_stress_node, in ms (zeros before the first call)
void stress_kernel_ms(MULTIGRID& g, double out[2]);

// the MULTIGRID behind a ddpca_multigrid_t (capi_multigrid.cpp); null for a null handle
MULTIGRID* multigrid_of(ddpca_multigrid_t h, bool* built);

// where an MCONTACT handle keeps resuDisp of its owned subdomain tv (device_mcontact.hip); false
// when tv is not owned by the handle's rank
struct SubDisp {
    int device = 0;
    hipStream_t stream = nullptr;
    const double* u_main = nullptr;
    const double* u_hang = nullptr;
    int64_t nn = 0, nh = 0;  // fine-level nodes, hanging-level dofs
};
bool mcontact_sub_disp(mcontact_t h, int64_t tv, SubDisp* out);

}  // namespace ddpca
