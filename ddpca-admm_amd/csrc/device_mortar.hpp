// The mortar operators of Interface::BUILD (MCONTACT.h:181-810, CONT_ROTA 157-179) on the device:
// the entry of device_mortar.hip.  No HIP type in this header.
#pragma once
#include "mortar_plan.hpp"

namespace ddpca {

// Builds `itf`'s nine operators per side, nodeCont, inpoNgap, pemaDiag and `factored` on the current
// device (selected by the caller): the plan on the host, uploads, k_mortar_pair, k_mortar_nodal and
// k_mortar_ip per side, copy back.  Every buffer lives for the call only; a failed allocation throws
// ApiError(DDPCA_EHIP) naming what was being allocated and its size.  No host fallback.
// ms: plan (host clock), uploads and allocations (host clock), k_mortar_pair, the two emit kernels
// together (HIP events, both sides), copy back (host clock).
void mortar_build_device(const MortarInput& in, Interface& itf, double ms[5]);

}  // namespace ddpca
