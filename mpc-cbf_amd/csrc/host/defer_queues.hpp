// defer_queues.hpp — the two deferral queues of an IMPC step, [count, -, agents ...] each, as word
// offsets into one zero-initialised buffer. The main launch appends the agents it defers to the
// current queue and zeroes the other one's header; the capacity launch behind it reads the current
// one; then the two change places. So the queue a launch appends to was zeroed by the launch before
// (or by the growth), whether or not a capacity launch ever read it.
// Decisions only, as grid_rotation.hpp: the owner of the buffer (capi.hip) passes the device calls in.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mpccbf {

class DeferQueues {
  public:
    static size_t bytes(int n) { return 2 * (size_t)(n + 2) * sizeof(int32_t); }

    // Room for n agents in each queue. Growth: alloc_zeroed(bytes) reallocates the buffer and zeroes
    // all of it (returns 0, or an error code that ensure returns: no capacity then, the next call
    // grows again), and the parity starts over.
    template <class AllocZeroed>
    int ensure(int n, AllocZeroed&& alloc_zeroed) {
        if (cap_ >= n) return 0;
        cap_ = 0;
        const int rc = alloc_zeroed(bytes(n));
        if (rc != 0) return rc;
        cap_ = n;
        parity_ = 0;
        return 0;
    }
    size_t current() const { return (size_t)parity_ * (cap_ + 2); }      // the main launch appends here
    size_t other() const { return (size_t)(parity_ ^ 1) * (cap_ + 2); }  // and zeroes this header
    // After the main launch, with whether it was enqueued: only then do the queues change places.
    // A launch that failed zeroed no header, so the next call must append to the same queue again.
    void advance(bool main_enqueued) {
        if (main_enqueued) parity_ ^= 1;
    }
    int capacity() const { return cap_; }

  private:
    int cap_ = 0, parity_ = 0;
};

}  // namespace mpccbf
