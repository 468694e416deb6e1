// Device-side plumbing every device source shares (device_common.hpp): the device check, the
// host-mapped stop state and the host's pacing of graph replays on it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <thread>

#include "../../include/ddpca_amd.h"
#include "device_common.hpp"

namespace ddpca {

void select_device(int device) {
    static thread_local int checked = -1;  // last device verified to be a gfx950 part
    if (device == checked) {
        DDPCA_HIP(hipSetDevice(device));
        return;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) throw ApiError(DDPCA_ENOGPU, "no HIP device visible");
    if (device < 0 || device >= n) throw ApiError(DDPCA_EINVAL, "device index out of range");
    DDPCA_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    DDPCA_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        throw ApiError(DDPCA_ENOGPU, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950");
    checked = device;
}

void MirrorBuf::alloc(int count) {
    n = count;
    DDPCA_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), std::max(1, count) * sizeof(PcgMirror),
                            hipHostMallocMapped | hipHostMallocCoherent));
    DDPCA_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), host, 0));
    reset();
}

void MirrorBuf::reset() { std::memset(host, 0, std::max(1, n) * sizeof(PcgMirror)); }

MirrorBuf::~MirrorBuf() {
    if (host) (void)hipHostFree(host);
}

// Host pacing of the parts' replays, one loop over all parts: a part keeps one replay of runway
// (it gets its next one when its slowest member has entered the last one enqueued for it); past
// its expected iteration count, single iterations kRunway ahead of the slowest member.
int64_t pace_parts(int np, hipStream_t* st, hipGraphExec_t* g, const MirrorBuf& m, const std::vector<int>& part, int64_t k,
                   int64_t launched0, hipGraphExec_t* g1, const int64_t* horizon) {
    constexpr int64_t kRunway = 2;  // tail: single iterations kept this far ahead of the slowest member
    if (np < 1 || np > kMaxParts) throw ApiError(DDPCA_EINVAL, "pace_parts: part count");
    int64_t launched[kMaxParts], replays = 0;
    for (int h = 0; h < np; ++h) launched[h] = launched0;
    for (int64_t spin = 0;; ++spin) {
        bool all = true;
        int64_t slowest[kMaxParts];
        bool busy[kMaxParts], tail[kMaxParts];
        for (int h = 0; h < np; ++h) slowest[h] = INT64_MAX, busy[h] = false;
        for (int s = 0; s < m.n; ++s) {
            if (__atomic_load_n(&m.host[s].done, __ATOMIC_ACQUIRE)) continue;
            all = false;
            busy[part[s]] = true;
            slowest[part[s]] = std::min<int64_t>(slowest[part[s]], __atomic_load_n(&m.host[s].iter, __ATOMIC_RELAXED));
        }
        if (all) return replays;
        bool launched_now = false;
        for (int h = 0; h < np; ++h) {
            tail[h] = g1 && horizon && g1[h] && launched[h] + k > horizon[h];
            if (busy[h] && (tail[h] ? launched[h] - slowest[h] <= kRunway : launched[h] - slowest[h] <= k)) {
                DDPCA_HIP(hipGraphLaunch(tail[h] ? g1[h] : g[h], st[h]));
                launched[h] += tail[h] ? 1 : k;
                ++replays;
                launched_now = true;
            }
        }
        if (launched_now) continue;
        if ((spin & 255) == 255) {
            for (int h = 0; h < np; ++h) {
                if (!busy[h]) continue;
                const hipError_t q = hipStreamQuery(st[h]);
                if (q == hipSuccess) {
                    // this part's stream drained: its mirror entries are final for what it ran
                    bool done_now = true;
                    for (int s = 0; s < m.n; ++s)
                        if (part[s] == h) done_now &= __atomic_load_n(&m.host[s].done, __ATOMIC_ACQUIRE) != 0;
                    if (!done_now) {
                        DDPCA_HIP(hipGraphLaunch(tail[h] ? g1[h] : g[h], st[h]));
                        launched[h] += tail[h] ? 1 : k;
                        ++replays;
                    }
                } else if (q != hipErrorNotReady) {
                    DDPCA_HIP(q);
                }
            }
        }
        std::this_thread::yield();
    }
}

// the whole batch on one stream: the loop of pace_parts for one part, kept apart -- merged into a
// one-part call it measured 0.3-0.6 % slower on a one-subdomain rank (the N = 8 layout), beyond the spread
int64_t pace_until_done(hipStream_t stream, hipGraphExec_t graph, const MirrorBuf& m, int64_t k, int64_t launched,
                        hipGraphExec_t graph1, int64_t horizon) {
    constexpr int64_t kRunway = 2;  // tail: single iterations kept this far ahead of the slowest member
    int64_t replays = 0;
    for (int64_t spin = 0;; ++spin) {
        bool all = true;
        int64_t slowest = INT64_MAX;
        for (int s = 0; s < m.n; ++s) {
            if (__atomic_load_n(&m.host[s].done, __ATOMIC_ACQUIRE)) continue;
            all = false;
            slowest = std::min<int64_t>(slowest, __atomic_load_n(&m.host[s].iter, __ATOMIC_RELAXED));
        }
        if (all) return replays;
        // keep one replay of runway: launch when the slowest solve has entered the last one;
        // past the expected iteration count, single iterations kRunway ahead
        const bool tail = graph1 && launched + k > horizon;
        if (tail ? launched - slowest <= kRunway : launched - slowest <= k) {
            DDPCA_HIP(hipGraphLaunch(tail ? graph1 : graph, stream));
            launched += tail ? 1 : k;
            ++replays;
            continue;
        }
        if ((spin & 255) == 255) {
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) {
                // stream drained: the mirror is final for everything enqueued so far
                bool done_now = true;
                for (int s = 0; s < m.n; ++s) done_now &= __atomic_load_n(&m.host[s].done, __ATOMIC_ACQUIRE) != 0;
                if (done_now) return replays;
                DDPCA_HIP(hipGraphLaunch(tail ? graph1 : graph, stream));
                launched += tail ? 1 : k;
                ++replays;
            } else if (q != hipErrorNotReady) {
                DDPCA_HIP(q);
            }
        }
        std::this_thread::yield();
    }
}

}  // namespace ddpca
