// Device stiffness assembly (device_stif.hip): the element loop of MULTIGRID::STIF_MATR,
// MULTIGRID.h:950-1039, and MULTIGRID::GET_VOLUME, MULTIGRID.h:1041-1082.  No HIP type in this
// header: the host translation units that reach the device path through a callback include it too.
#pragma once
#include <cstdint>
#include <functional>

#include "../../include/ddpca_amd.h"
#include "multigrid.hpp"

namespace ddpca {

// The values of g's nodal stiffness on `device` (current, selected by the caller) into val, 9
// doubles per stored block of the pattern g.STIF_PLAN().K, and the volume of the leaf elements
// (volume may be null).  The plan's device copy is uploaded on the first call and kept with g
// (StifPlan::device); the element scratch (kStifElemDoubles doubles per leaf element) lives for the
// call only, and a failed allocation throws with the size it needed.  Synchronous: returns after
// the copy back.  ms (may be null): HIP-event times of k_stif_elem and k_stif_gather, then the
// host clock of the plan upload (0 when cached) and of the copy back.
void stif_device(MULTIGRID& g, int device, double* val, double* volume, double ms[4]);

// GET_VOLUME alone: the element kernel without the stiffness accumulators, then the reduction.
double volume_device(MULTIGRID& g, int device);

// ddpca_multigrid_build with STIF_MATR's element loop left to `values` when given
// and CONSTRAINT's Galerkin chain left to `galerkin` when given (capi_multigrid.cpp; throws ApiError)
void multigrid_build(ddpca_multigrid_t h, const ddpca_csr_t* extra, const std::function<void(MULTIGRID&, double* val)>* values,
                     const GalerkinChain* galerkin = nullptr);

// the element loop of STIF_MATR on `device` as STIF_MATR_BY takes it (capi_stif.hip: it selects the
// device, builds the plan when g has none and keeps the times of ddpca_stif_last_*_ms)
std::function<void(MULTIGRID&, double* val)> stif_device_values(int device);

constexpr int kStifElemDoubles = 576;  // 8 x 8 blocks of 9, every block stored (no symmetry)

}  // namespace ddpca
