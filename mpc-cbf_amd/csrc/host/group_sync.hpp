// group_sync.hpp — how the ranks of an in-process communicator group (mpccbf_comm_create_local:
// host threads of one process) wait for each other inside mpccbf_run_steps: a barrier that an
// aborting rank breaks for good, the agreement on num_steps at a call's entry, and the guard that
// aborts when a rank leaves a call early. Plain C++: no HIP call. The owner of the group's device
// half (capi_run.hip, LocalGroup: the per-step tables and events) builds on it;
// tools/run_owners_check.cpp drives the same class from real threads (tests/test_run_owners.py).
#pragma once

#include <condition_variable>
#include <mutex>
#include <vector>

namespace mpccbf {

class GroupSync {
  public:
    explicit GroupSync(int nranks) : nranks_(nranks), counts_(nranks, 0) {}
    int nranks() const { return nranks_; }

    // Returns once every rank has arrived: true. false: a rank aborted, before this call or while
    // it waited. From then on every barrier fails at once: the group cannot be used again
    // (destroy and recreate it).
    bool barrier() {
        std::unique_lock<std::mutex> lk(m_);
        return arrive(lk);
    }
    void abort() {
        std::lock_guard<std::mutex> lk(m_);
        aborted_ = true;
        cv_.notify_all();
    }

    // Every rank enters a call with its count (num_steps): a barrier after which each rank knows
    // whether all the counts are equal.
    enum Agreement { ABORTED, DIFFERS, SAME };
    // Why every rank gets the verdict of its own generation, whatever a rank that races ahead into
    // its next call does. A count is written in the critical section in which its rank arrives,
    // and the counts are compared by the generation's last arriver alone, in the critical section
    // that completes the generation: after every rank's write of this generation, and before any
    // write of the next, which needs its writer to have left this barrier. The verdict is
    // overwritten only by the last arriver of the next generation, hence after every rank has
    // left this one, and a waiter reads it before it leaves, under the mutex it wakes up with.
    Agreement agree(int rank, int count) {
        std::unique_lock<std::mutex> lk(m_);
        counts_[rank] = count;
        if (!arrive(lk)) return ABORTED;
        return same_ ? SAME : DIFFERS;
    }

  private:
    bool arrive(std::unique_lock<std::mutex>& lk) {
        if (aborted_) return false;
        const long long g = gen_;
        if (++arrived_ == nranks_) {
            same_ = true;
            for (int v : counts_) same_ = same_ && v == counts_[0];
            arrived_ = 0;
            gen_++;
            cv_.notify_all();
            return true;
        }
        cv_.wait(lk, [&] { return gen_ != g || aborted_; });
        return gen_ != g;
    }

    const int nranks_;
    std::mutex m_;
    std::condition_variable cv_;
    int arrived_ = 0;
    long long gen_ = 0;
    bool aborted_ = false;
    std::vector<int> counts_;  // [rank]: the count of its last agree()
    bool same_ = true;         // the counts of the last completed generation were equal
};

// Aborts the group when it leaves scope armed: a rank that returns from mpccbf_run_steps before its
// last barrier makes the peers' barriers fail, where they would wait forever. g: null for none.
struct GroupAbortGuard {
    GroupSync* g = nullptr;
    explicit GroupAbortGuard(GroupSync* group) : g(group) {}
    GroupAbortGuard(const GroupAbortGuard&) = delete;
    GroupAbortGuard& operator=(const GroupAbortGuard&) = delete;
    void disarm() { g = nullptr; }
    ~GroupAbortGuard() {
        if (g) g->abort();
    }
};

}  // namespace mpccbf
