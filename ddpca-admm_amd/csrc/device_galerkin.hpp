// Device Galerkin products (device_galerkin.hip): the chain of MULTIGRID::CONSTRAINT,
// MULTIGRID.h:1182-1184, levelStif[l] = P_l^T levelStif[l + 1] P_l, on the pattern of
// galerkin_pattern (sparse.cpp; the pattern is the host's own).  No HIP type in this header: the
// host translation units reach the device path only through MULTIGRID::galerkinChain.
#pragma once
#include <cstdint>
#include <vector>

#include "sparse.hpp"

namespace ddpca {

// out[i] = chain[i]^T (out[i - 1], or K for i = 0) chain[i] on `device` (current, selected by the
// caller): the patterns on the host (before the lock), then under one process-wide lock the
// finest values uploaded once, product after product by k_rap with each level's result feeding the
// next on the device, every level's values copied back into out[i] (ptr / col: the pattern's) and
// a finer level's device copy freed once its product is done.  A stencil with block entries takes
// the block instance of the kernel, as galerkin_rap chooses by S.bent.empty().  Synchronous.  A
// failed allocation throws DDPCA_EHIP with the size it needed; there is no host fallback.
// ms (may be null): host clock of the pattern build and of the uploads, HIP-event time of the
// kernels summed over the levels, host clock of the copies back (with the sizing of the host
// arrays they fill, done before the lock); level_ms (may be null): the kernel time of each product.
void galerkin_chain_device(int device, const Bsr3& K, const std::vector<const Stencil*>& chain, std::vector<Bsr3>& out,
                           double ms[4], std::vector<double>* level_ms = nullptr);

}  // namespace ddpca
