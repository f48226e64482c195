// run_owners_check.cpp — the two owners behind mpccbf_run_steps that decide without a device: the
// in-process group's synchronisation (csrc/host/group_sync.hpp) driven from real threads, and the
// timing events' layout (csrc/host/step_events.hpp) over every small call. Plain C++ and threads:
// no HIP, no library. Built by the Makefile as build/run_owners_check and run by
// tests/test_run_owners.py; the Makefile also builds it under the thread sanitizer and under the
// address / undefined-behaviour sanitizers (run_owners_tsan, run_owners_asan).
//
// The assertions are a model's, kept here, not the classes':
//   group   arrivals[g] counts the ranks that have reached their g-th barrier. A rank adds itself
//           before it enters and, when the barrier lets it through, must find every rank counted:
//           no thread leaves generation g before all have arrived.
//           1. over many generations every barrier returns true on every rank
//           2. agree() says SAME on every rank when the counts are equal and DIFFERS on every rank
//              when one differs, over back-to-back calls whose counts change every time (a rank
//              that runs ahead into its next call must not change what a slower rank is told)
//           3. the zero-step call of mpccbf_run_steps (agree, barrier, guard disarmed) leaves the
//              group usable
//           4. an abort (a) before the others arrive, (b) while they wait, (c) between two
//              barriers, by a guard that leaves scope armed: every other rank's current and later
//              barriers and agreements fail, and nobody blocks (a hang is the caller's timeout)
//           5. the slot discipline of the group's device half (capi_run.hip, exchange_local), with
//              integers for the tables and events: what rank p put into slot s & 1 before step s's
//              barrier is what its peers read after it, and p writes that slot again only after
//              the barrier of step s + 1. The slots are plain ints, so under the thread sanitizer
//              a write that a barrier does not order against a read is a reported race.
//   events  the driver records and reads events in capi_run.hip's order (start_timing, the step
//           loop, read_timings) for num_steps 0..6, reserve_steps 0..8, solve_stride 0..4 and
//           step_ms / solve_ms given or not:
//           6. every event read or waited for was recorded earlier in the call and lies below
//              needed(); a step's roles are distinct events; no event is recorded twice
//           7. step intervals are contiguous from the start event
//           8. with any timing the last step's end is recorded, last, and is the one waited for
//           9. solve_ms[s] is a pair exactly when solve_stride <= 1 or s % solve_stride == 0
//          10. without timing nothing is recorded, waited for or read
//          11. needed() == 3 * max(num_steps, reserve_steps) + 1
#include <atomic>
#include <chrono>
#include <cstdio>
#include <functional>
#include <set>
#include <thread>
#include <vector>

#include "group_sync.hpp"
#include "step_events.hpp"

using namespace mpccbf;

namespace {

std::atomic<long> failures{0}, barriers{0}, agreements{0}, aborts_seen{0}, slot_reads{0};
long plans = 0;

void check(bool ok, const char* what, int a = 0, int b = 0) {
    if (ok) return;
    if (failures++ < 20) std::printf("FAIL: %s (%d, %d)\n", what, a, b);
}

void run_ranks(int n, const std::function<void(int)>& body) {
    std::vector<std::thread> th;
    for (int r = 0; r < n; r++) th.emplace_back(body, r);
    for (auto& t : th) t.join();
}

// ---- the group --------------------------------------------------------------------------------

// The model next to one GroupSync: per-generation arrival counts
struct Group {
    GroupSync sync;
    std::vector<std::atomic<int>> arrivals;
    Group(int n, int generations) : sync(n), arrivals(generations) {
        for (auto& a : arrivals) a = 0;
    }
    void arrive(int g) { arrivals[g]++; }
    // a barrier or agreement of generation g let this rank through
    void passed(int g) {
        check(arrivals[g] == sync.nranks(), "a rank left a generation before all had arrived", g, arrivals[g]);
        barriers++;
    }
    bool barrier(int g) {
        arrive(g);
        const bool ok = sync.barrier();
        if (ok) passed(g);
        return ok;
    }
    GroupSync::Agreement agree(int g, int rank, int count) {
        arrive(g);
        const GroupSync::Agreement a = sync.agree(rank, count);
        if (a != GroupSync::ABORTED) passed(g);
        return a;
    }
};

constexpr int GENERATIONS = 2000;

void many_barriers(int n) {
    Group w(n, GENERATIONS);
    run_ranks(n, [&](int) {
        for (int g = 0; g < GENERATIONS; g++) check(w.barrier(g), "1: a barrier of a sound group failed", n, g);
    });
}

// back-to-back agreements: call k's count is 5 + k % 7 on every rank, but on rank k % n of every
// third call it is one more
void many_agreements(int n) {
    Group w(n, GENERATIONS);
    run_ranks(n, [&](int rank) {
        for (int k = 0; k < GENERATIONS; k++) {
            const bool differs = k % 3 == 1;
            const int count = 5 + k % 7 + (differs && rank == k % n ? 1 : 0);
            const GroupSync::Agreement a = w.agree(k, rank, count);
            check(a == (differs ? GroupSync::DIFFERS : GroupSync::SAME), "2: the verdict of an agreement", n, k);
            agreements++;
        }
    });
}

// mpccbf_run_steps with num_steps == 0, then with one step whose exchange is a barrier
void zero_step_calls(int n) {
    constexpr int CALLS = 50;
    Group w(n, 4 * CALLS);
    run_ranks(n, [&](int rank) {
        int g = 0;
        for (int call = 0; call < CALLS; call++) {
            {
                GroupAbortGuard guard(&w.sync);
                check(w.agree(g++, rank, 0) == GroupSync::SAME, "3: the zero-step agreement", n, call);
                check(w.barrier(g++), "3: the zero-step call's barrier", n, call);
                guard.disarm();
            }
            {
                GroupAbortGuard guard(&w.sync);
                check(w.agree(g++, rank, 1) == GroupSync::SAME, "3: the agreement after a zero-step call", n, call);
                check(w.barrier(g++), "3: a disarmed guard aborted the group", n, call);
                guard.disarm();
            }
        }
    });
}

enum AbortCase { BEFORE_ARRIVAL, WHILE_WAITING, BETWEEN_BARRIERS };

// rank `who` aborts; the others' current barrier, the next one and the next agreement fail
void abort_case(int n, AbortCase c, int who) {
    Group w(n, 4);
    std::atomic<bool> aborted{false};
    run_ranks(n, [&](int rank) {
        int g = 0;
        if (c == BETWEEN_BARRIERS) check(w.barrier(g++), "4c: the barrier before the abort", n, rank);
        if (rank == who) {
            if (c == WHILE_WAITING) {  // the peers have announced themselves and are in the barrier or about to be
                while (w.arrivals[g] < n - 1) std::this_thread::yield();
                std::this_thread::sleep_for(std::chrono::milliseconds(2));
            }
            {
                GroupAbortGuard guard(&w.sync);  // leaves scope armed
            }
            aborted = true;
            return;
        }
        if (c == BEFORE_ARRIVAL)
            while (!aborted) std::this_thread::yield();
        check(!w.barrier(g++), "4: a barrier passed although a rank aborted", n, (int)c);
        check(!w.barrier(g++), "4: a later barrier passed after an abort", n, (int)c);
        check(w.agree(g++, rank, 3) == GroupSync::ABORTED, "4: an agreement after an abort", n, (int)c);
        aborts_seen++;
    });
}

// exchange_local's order with integers: publish, barrier, read every peer's slot of the step
void slot_discipline(int n) {
    constexpr int STEPS = 500;
    Group w(n, STEPS);
    std::vector<int> slot[2] = {std::vector<int>(n, -1), std::vector<int>(n, -1)};
    auto value = [](int rank, int s) { return 1000 * s + rank; };
    run_ranks(n, [&](int rank) {
        for (int s = 0; s < STEPS; s++) {
            slot[s & 1][rank] = value(rank, s);
            if (!w.barrier(s)) return check(false, "5: a step's barrier failed", n, s);
            for (int p = 0; p < n; p++) {
                if (p == rank) continue;
                check(slot[s & 1][p] == value(p, s), "5: a peer's slot does not hold its step's table", s, p);
                slot_reads++;
            }
        }
    });
}

// ---- the timing events ------------------------------------------------------------------------

// One call of mpccbf_run_steps as far as its events go
struct EventModel {
    const StepEvents& plan;
    std::vector<int> order;  // [event]: when it was recorded (1, 2, ...), 0: not in this call
    int clock = 0;
    explicit EventModel(const StepEvents& p) : plan(p), order(p.needed() > 0 ? p.needed() : 0, 0) {}

    bool inside(int e) const { return e >= 0 && e < (int)order.size(); }
    void record(int e) {
        check(inside(e), "6: an event outside the pool is recorded", e, plan.needed());
        if (!inside(e)) return;
        check(order[e] == 0, "6: an event is recorded twice", e);
        order[e] = ++clock;
    }
    bool readable(int e, int before) const { return inside(e) && order[e] > 0 && order[e] <= before; }
};

void event_plan(int steps, int reserve, int stride, bool step_ms, bool solve_ms) {
    const StepEvents plan(steps, reserve, stride, step_ms, solve_ms);
    const bool timing = step_ms || solve_ms;
    plans++;
    check(plan.needed() == 3 * (steps > reserve ? steps : reserve) + 1, "11: needed()", steps, reserve);
    check(plan.timing() == timing, "timing()");
    EventModel m(plan);
    // the roles
    std::set<int> roles{plan.start()};
    for (int s = 0; s < steps; s++)
        for (int e : {plan.solve_begin(s), plan.solve_end(s), plan.step_end(s)}) {
            check(m.inside(e), "6: a role outside the pool", s, e);
            check(roles.insert(e).second, "6: two roles share an event", s, e);
        }
    // start_timing, the step loop
    if (plan.records_start()) m.record(plan.start());
    for (int s = 0; s < steps; s++) {
        if (plan.times_solve(s)) {
            m.record(plan.solve_begin(s));
            m.record(plan.solve_end(s));
        }
        if (plan.records_end(s)) m.record(plan.step_end(s));
    }
    if (!timing) check(m.clock == 0 && plan.waits_for() < 0, "10: an untimed call records or waits", steps, stride);
    // read_timings
    const int last = plan.waits_for();
    if (timing && steps > 0) {
        check(last == plan.step_end(steps - 1), "8: the call does not wait for the last step's end", steps, last);
        check(m.inside(last) && m.order[last] == m.clock, "8: the event waited for is not the last recorded", steps, last);
    } else {
        check(last < 0, "8: a call without a timed step waits", steps, last);
    }
    if (last < 0 || !m.inside(last)) return;
    const int done = m.order[last];
    for (int s = 0; s < steps; s++) {
        if (step_ms) {
            const StepEvents::Pair p = plan.step_slot(s);
            check(m.readable(p.from, done) && m.readable(p.to, done) && m.order[p.from] < m.order[p.to],
                  "6: step_ms reads an event that was not recorded in order", s, p.from);
            check(p.to == plan.step_end(s), "7: a step's interval does not end at its end event", s, p.to);
            check(p.from == (s == 0 ? plan.start() : plan.step_slot(s - 1).to), "7: step intervals are not contiguous", s,
                  p.from);
        }
        if (solve_ms) {
            const StepEvents::Pair p = plan.solve_slot(s);
            const bool timed = stride <= 1 || s % stride == 0;
            check((p.from >= 0) == timed, "9: the steps whose solve is timed", s, stride);
            if (p.from >= 0)
                check(p.from == plan.solve_begin(s) && p.to == plan.solve_end(s) && m.readable(p.from, done) &&
                          m.readable(p.to, done) && m.order[p.from] < m.order[p.to],
                      "6: solve_ms reads an event that was not recorded in order", s, p.from);
        }
    }
}

}  // namespace

int main() {
    for (int n : {2, 3, 8}) {
        many_barriers(n);
        many_agreements(n);
        zero_step_calls(n);
        for (AbortCase c : {BEFORE_ARRIVAL, WHILE_WAITING, BETWEEN_BARRIERS})
            for (int who : {0, n - 1}) abort_case(n, c, who);
        slot_discipline(n);
    }
    for (int steps = 0; steps <= 6; steps++)
        for (int reserve = 0; reserve <= 8; reserve++)
            for (int stride = 0; stride <= 4; stride++)
                for (int given = 0; given < 4; given++) event_plan(steps, reserve, stride, given & 1, given & 2);
    std::printf("run_owners_check: %ld barriers, %ld agreements, %ld aborted ranks, %ld slot reads, %ld event plans, "
                "%ld failures\n",
                barriers.load(), agreements.load(), aborts_seen.load(), slot_reads.load(), plans, failures.load());
    return failures ? 1 : 0;
}
