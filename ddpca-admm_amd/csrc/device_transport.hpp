// The exchanges of a multi-rank run, all stream-ordered on the rank's stream:
//   exchange()      the gamma halves of cross-rank interfaces (one grouped send/recv per peer)
//   allreduce_sum() the MONITOR norms and the coarse right-hand side every iteration, the dense
//                   coarse matrix once at setup
// The RCCL transport is the production path (RCCL over xGMI); the local transports connect the
// handles of ONE process through host-staged copies (mcontact_gpu_comm_local) so the multi-rank
// bookkeeping (owner maps, gamma offsets, rank-local coarse rows) runs on a single GPU in the tests.
// Implementations: device_transport.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

namespace ddpca {

struct Transport {
    struct Msg {
        int peer;
        int64_t tag;  // interface index
        const double* send;
        double* recv;
        int64_t n;
    };
    virtual ~Transport() = default;
    virtual void allreduce_sum(double* buf, int64_t n, hipStream_t st) = 0;
    virtual void exchange(const std::vector<Msg>& msgs, hipStream_t st) = 0;
};

// RCCL: a fresh unique id (128 bytes, what rank 0 hands every rank), and rank `rank` of the
// communicator of `nranks` built from it (collective)
void rccl_unique_id(void* out128);
std::unique_ptr<Transport> rccl_transport(int nranks, int rank, const void* uid128);

// Timing-only transport (mcontact_gpu_comm_loopback): every receive from peer p gets what this
// rank sent p, as an on-device copy on the solve stream; all-reduces keep this rank's own values.
// One rank of an N-rank layout then runs its own share of the work on a single GPU.
std::unique_ptr<Transport> loopback_transport();

// The n connected transports of one process's ranks (rank r at [r]; each rank's calls come from
// its own host thread)
std::vector<std::unique_ptr<Transport>> local_transports(int n);

}  // namespace ddpca
