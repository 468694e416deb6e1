// The rank transports (device_transport.hpp): RCCL, loopback, and the in-process local hub.
#include "device_transport.hpp"

#include <rccl/rccl.h>

#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <string>

#include "../../include/ddpca_amd.h"
#include "device_common.hpp"

namespace ddpca {

namespace {

#define DDPCA_NCCL(call)                                                                                  \
    do {                                                                                                  \
        ncclResult_t r_ = (call);                                                                         \
        if (r_ != ncclSuccess) throw ApiError(DDPCA_ECOMM, std::string(#call) + ": " + ncclGetErrorString(r_)); \
    } while (0)

static_assert(sizeof(ncclUniqueId) == 128, "the C ABI hands the unique id over as 128 bytes");

struct RcclTransport : Transport {
    ncclComm_t comm = nullptr;
    ~RcclTransport() override {
        if (comm) (void)ncclCommDestroy(comm);
    }
    void allreduce_sum(double* buf, int64_t n, hipStream_t st) override {
        DDPCA_NCCL(ncclAllReduce(buf, buf, (size_t)n, ncclDouble, ncclSum, comm, st));
    }
    void exchange(const std::vector<Msg>& msgs, hipStream_t st) override {
        DDPCA_NCCL(ncclGroupStart());
        for (const Msg& m : msgs) {
            DDPCA_NCCL(ncclSend(m.send, (size_t)m.n, ncclDouble, m.peer, comm, st));
            DDPCA_NCCL(ncclRecv(m.recv, (size_t)m.n, ncclDouble, m.peer, comm, st));
        }
        DDPCA_NCCL(ncclGroupEnd());
    }
};

struct LoopbackTransport : Transport {
    void allreduce_sum(double*, int64_t, hipStream_t) override {}
    void exchange(const std::vector<Msg>& msgs, hipStream_t st) override {
        for (const Msg& m : msgs)
            if (m.n) DDPCA_HIP(hipMemcpyAsync(m.recv, m.send, (size_t)m.n * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
};

// Rendezvous of the ranks of one process (each rank's calls come from its own host thread).
struct LocalHub {
    int n = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    int64_t generation = 0;
    bool broken = false;
    std::vector<std::vector<double>> slot;  // allreduce staging per rank
    // posted sends per (src, dst) in issue order -- matched against the receiver's receives from
    // src in ITS issue order, as RCCL matches grouped ncclSend / ncclRecv pairs per peer (tags and
    // sizes are only checked, never used for matching: an ordering bug fails here as on the wire)
    struct Posted {
        int64_t tag;
        const double* buf;
        int64_t n;
    };
    std::map<std::pair<int, int>, std::deque<Posted>> post;
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        if (broken) throw ApiError(DDPCA_ECOMM, "local transport: a peer failed");
        const int64_t g = generation;
        if (++arrived == n) {
            arrived = 0;
            ++generation;
            cv.notify_all();
        } else if (!cv.wait_for(lk, std::chrono::seconds(120), [&] { return generation != g || broken; }) || broken) {
            broken = true;
            cv.notify_all();
            throw ApiError(DDPCA_ECOMM, "local transport: peers did not arrive");
        }
    }
};

struct LocalTransport : Transport {
    std::shared_ptr<LocalHub> hub;
    int rank = 0;
    void allreduce_sum(double* buf, int64_t n, hipStream_t st) override {
        auto& mine = hub->slot[rank];
        mine.resize(n);
        DDPCA_HIP(hipMemcpyAsync(mine.data(), buf, n * sizeof(double), hipMemcpyDeviceToHost, st));
        DDPCA_HIP(hipStreamSynchronize(st));
        hub->barrier();
        std::vector<double> sum(n, 0.0);
        for (int q = 0; q < hub->n; ++q)  // rank order: every rank gets the same bits
            for (int64_t i = 0; i < n; ++i) sum[i] += hub->slot[q][i];
        DDPCA_HIP(hipMemcpyAsync(buf, sum.data(), n * sizeof(double), hipMemcpyHostToDevice, st));
        DDPCA_HIP(hipStreamSynchronize(st));
        hub->barrier();  // nobody restages before every rank has read the slots
    }
    void exchange(const std::vector<Msg>& msgs, hipStream_t st) override {
        DDPCA_HIP(hipStreamSynchronize(st));
        {
            std::lock_guard<std::mutex> lk(hub->mu);
            for (const Msg& m : msgs) hub->post[{rank, m.peer}].push_back({m.tag, m.send, m.n});
        }
        hub->barrier();
        std::string err;
        for (const Msg& m : msgs) {
            LocalHub::Posted p{};
            {
                std::lock_guard<std::mutex> lk(hub->mu);
                auto& q = hub->post[{m.peer, rank}];
                if (q.empty()) {
                    err = "local transport: receive from rank " + std::to_string(m.peer) + " has no matching send";
                    break;
                }
                p = q.front();
                q.pop_front();
            }
            if (p.tag != m.tag || p.n != m.n) {
                err = "local transport: message order differs between ranks " + std::to_string(m.peer) + " and " +
                      std::to_string(rank) + " (tag " + std::to_string(p.tag) + " sent, " + std::to_string(m.tag) +
                      " expected)";
                break;
            }
            DDPCA_HIP(hipMemcpyAsync(m.recv, p.buf, m.n * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        DDPCA_HIP(hipStreamSynchronize(st));
        if (!err.empty()) {
            std::lock_guard<std::mutex> lk(hub->mu);
            hub->broken = true;
            hub->cv.notify_all();
            throw ApiError(DDPCA_ECOMM, err);
        }
        hub->barrier();  // the peers' send buffers stay untouched until every copy has landed
        std::lock_guard<std::mutex> lk(hub->mu);
        for (const Msg& m : msgs)
            if (!hub->post[{rank, m.peer}].empty()) {
                hub->broken = true;
                throw ApiError(DDPCA_ECOMM, "local transport: a send to rank " + std::to_string(m.peer) + " was not received");
            }
    }
};

}  // namespace

void rccl_unique_id(void* out128) {
    ncclUniqueId id;
    DDPCA_NCCL(ncclGetUniqueId(&id));
    std::memcpy(out128, &id, sizeof(id));
}

std::unique_ptr<Transport> rccl_transport(int nranks, int rank, const void* uid128) {
    ncclUniqueId id;
    std::memcpy(&id, uid128, sizeof(id));
    auto t = std::make_unique<RcclTransport>();
    DDPCA_NCCL(ncclCommInitRank(&t->comm, nranks, id, rank));
    return t;
}

std::unique_ptr<Transport> loopback_transport() { return std::make_unique<LoopbackTransport>(); }

std::vector<std::unique_ptr<Transport>> local_transports(int n) {
    auto hub = std::make_shared<LocalHub>();
    hub->n = n;
    hub->slot.resize(n);
    std::vector<std::unique_ptr<Transport>> out;
    for (int r = 0; r < n; ++r) {
        auto t = std::make_unique<LocalTransport>();
        t->hub = hub;
        t->rank = r;
        out.push_back(std::move(t));
    }
    return out;
}

}  // namespace ddpca
