// host_state_check.cpp — the neighbour-table rotation (csrc/host/grid_rotation.hpp) and the deferral
// queues (csrc/host/defer_queues.hpp) over every sequence of up to four calls on one context, next
// to a model of what the device buffers hold. Plain C++: no HIP, no library. Built by the Makefile
// as build/host_state_check and run by tests/test_host_state.py.
//
// The driver below makes the calls of capi.hip (impc_enqueue), capi_run.hip (mpccbf_run_steps) and
// capi_ctx.hpp (GridTables::carve / rebuild) on GridRotation and DeferQueues in their order, and
// where they enqueue device work it applies that work's effect to the model:
//   a neighbour table holds   ZERO | COPY of state version v | DIRTY | GONE (reallocated, or never there)
//   a deferral queue's header ZERO | DIRTY | GONE
//   a state table holds a version; every kernel that writes one, and every caller that may have,
//   gives it a new one.
// The assertions are the model's, not the classes': they hold whatever rule the classes follow.
//   1. every grid step reads a table that holds a COPY of the version of the state table it is given
//   2. every step of a rotation inserts into a ZERO table, and its three roles are distinct
//   3. a call that must not continue (anything but a completed grid run came before it, or its
//      query differs) rebuilds
//   4. a call that may continue does, with no rebuild
//   5. the queue a main launch appends to is ZERO, is not the one it zeroes, and both lie inside
//      the buffer; growth leaves both ZERO; a main launch that failed moves nothing
#include <cstdio>
#include <string>
#include <vector>

#include "defer_queues.hpp"
#include "grid_rotation.hpp"

using namespace mpccbf;

namespace {

enum Kind { ZERO, COPY, DIRTY, GONE };
struct Table {
    Kind kind = GONE;
    int ver = 0;
};

// the model's table size (capi_ctx.hpp: grid_table_bytes; any function that grows with the power of
// two >= num_states, from 1024 buckets, serves)
unsigned table_size(int ns) {
    unsigned T = 1024;
    while (T < (unsigned)ns) T <<= 1;
    return T;
}
size_t table_bytes(int ns) { return (size_t)table_size(ns) * 100; }

struct Call {
    const char* name;
    int steps;        // run: steps; < 0: a single mpccbf_impc_solve
    bool csr;
    bool cont;        // mpccbf_run::continue_tables
    int ns = 1024, k = 8;
    double radius = 1.0;
    bool refill = false;      // the caller rewrites the state table before the call
    int fail_step = -1;       // the main launch of this step fails
    bool alloc_fails = false; // a growth of the neighbour tables' buffer fails
};

const Call ALPHABET[] = {
    {"grid1", 1, false, false},
    {"grid1c", 1, false, true},
    {"grid2", 2, false, false},
    {"grid2c", 2, false, true},
    {"grid3", 3, false, false},
    {"grid3c", 3, false, true},
    {"csr2", 2, true, true},
    {"solve", -1, false, false},
    {"solve_csr", -1, true, false},
    {"zero", 0, false, true},
    {"zero_refill", 0, false, true, 1024, 8, 1.0, true},
    {"grid1c_ns1025", 1, false, true, 1025},
    {"grid1c_k9", 1, false, true, 1024, 9},
    {"grid1c_r2", 1, false, true, 1024, 8, 2.0},
    {"grid2c_fail1", 2, false, true, 1024, 8, 1.0, false, 1},
    {"grid1c_ns1025_noalloc", 1, false, true, 1025, 8, 1.0, false, -1, true},
};
constexpr int LETTERS = sizeof(ALPHABET) / sizeof(ALPHABET[0]);

long failures = 0, steps_run = 0, continued = 0, rebuilt = 0, grown = 0;
std::string current_sequence;

void check(bool ok, const char* what) {
    if (ok) return;
    if (failures++ < 20) std::printf("FAIL [%s]: %s\n", current_sequence.c_str(), what);
}

// One context and the device memory behind it
struct World {
    // ---- what the context holds ----
    GridRotation rot;
    DeferQueues queues;
    size_t grid_bytes = 0;  // GridTables::buf.bytes
    // ---- the model ----
    Table table[3];
    unsigned carved = 0;    // table size of the last carve: another one moves the tables in the buffer
    Kind queue[2] = {GONE, GONE};
    double state_mem[2] = {};
    int ver[2] = {1, 2}, next_ver = 3;
    int cur = 0;            // the state table the caller passes next
    // what the call before left to continue, by the API's rule (mpccbf.h, continue_tables): set by a
    // grid run that enqueued every step, taken by the next call of any kind
    bool may = false;
    GridQuery may_q{};

    const double* ptr(int t) const { return &state_mem[t]; }

    // GridTables::carve
    bool carve(const Call& c) {
        const size_t need = 3 * table_bytes(c.ns);
        rot.reallocates(need, grid_bytes);
        if (need > grid_bytes) {  // DevBuf::reserve
            grid_bytes = 0;
            for (Table& t : table) t.kind = GONE;
            if (c.alloc_fails) return false;
            grid_bytes = need;
        }
        if (carved != table_size(c.ns))
            for (Table& t : table)
                if (t.kind != GONE) t.kind = DIRTY;
        carved = table_size(c.ns);
        return true;
    }
    // GridTables::rebuild
    void rebuild(int states, bool zero_fill) {
        table[0] = Table{COPY, ver[states]};
        if (zero_fill) table[1] = Table{ZERO, 0};
        rebuilt++;
    }

    // impc_enqueue: the step reads state table `in` and writes `out` (-1: nowhere the model follows)
    bool enqueue(const Call& c, int run_step, int in, int out, bool fail) {
        const GridRoles roles = run_step < 0 ? rot.foreign_step() : rot.step(run_step);
        if (!c.csr) {  // grid_args
            if (!carve(c)) return false;
            if (roles.fill < 0) {
                rebuild(in, false);
            } else {
                check(roles.read != roles.fill && roles.fill != roles.zero && roles.zero != roles.read &&
                          roles.read >= 0 && roles.read < 3 && roles.fill >= 0 && roles.fill < 3 && roles.zero >= 0 &&
                          roles.zero < 3,
                      "2: the three roles are not three tables");
                if (roles.fill < 0 || roles.fill > 2 || roles.zero < 0 || roles.zero > 2) return false;
                check(table[roles.fill].kind == ZERO, "2: the step inserts into a table that is not zero");
            }
            if (roles.read < 0 || roles.read > 2) return false;
            check(table[roles.read].kind == COPY && table[roles.read].ver == ver[in],
                  "1: the step reads a table that does not hold its states");
        }
        // defer_args
        const int n = c.ns;
        const bool grows = queues.capacity() < n;
        const int rc = queues.ensure(n, [&](size_t bytes) {
            check(bytes == DeferQueues::bytes(n), "5: growth to another size than the queues need");
            queue[0] = queue[1] = ZERO;  // (reserve + memset of the whole buffer)
            grown++;
            return 0;
        });
        check(rc == 0, "5: ensure failed");
        const size_t q = queues.current(), o = queues.other(), words = DeferQueues::bytes(queues.capacity()) / 4;
        check(queues.capacity() >= n, "5: no room for the batch");
        check(q != o && (q == 0 || o == 0) && q + n + 2 <= words && o + n + 2 <= words &&
                  (q < o ? q + n + 2 <= o : o + n + 2 <= q),
              "5: the queues overlap or leave the buffer");
        if (grows) check(queue[0] == ZERO && queue[1] == ZERO && q == 0, "5: growth did not zero both queues");
        const int qi = q == 0 ? 0 : 1;
        check(queue[qi] == ZERO, "5: the main launch appends to a queue that was not zeroed");
        // main launch
        if (!fail) {
            queue[qi] = DIRTY;
            queue[qi ^ 1] = ZERO;
            if (!c.csr && roles.fill >= 0) {
                table[roles.zero] = Table{ZERO, 0};
                table[roles.fill] = Table{COPY, next_ver};  // (with the rows of mpccbf_run_steps' insert)
            }
            if (out >= 0) ver[out] = next_ver;
            next_ver++;
            steps_run++;
        }
        queues.advance(!fail);
        if (fail) check(queues.current() == q, "5: a failed main launch moved the queues");
        return !fail;  // (the capacity launch reads queue qi and writes no state the model follows)
    }

    // mpccbf_impc_solve: where its caller points next_states is its own business, so the state table
    // counts as rewritten afterwards
    void solve(const Call& c) {
        enqueue(c, -1, cur, -1, false);
        ver[cur] = next_ver++;
    }

    // mpccbf_run_steps with states = the table the last run ended in, states_alt = the other
    void run(const Call& c, bool may_now, const GridQuery& may_was) {
        const int tables[2] = {cur, cur ^ 1};
        const bool gtab = !c.csr && c.steps > 0;  // (count > 0 throughout)
        const GridQuery q{ptr(cur), c.ns, 0, c.ns, c.k, c.radius};
        if (!gtab) rot.no_rotation();
        if (gtab) {
            if (!carve(c)) return;
            const bool same = may_was.states == q.states && may_was.ns == q.ns && may_was.first == q.first &&
                              may_was.count == q.count && may_was.k == q.k && may_was.radius == q.radius;
            const bool expect = c.cont && may_now && same;
            const int base = rot.run_started(q, c.cont);
            check(!(base >= 0 && !expect), "3: the call continues across an event or with another query");
            check(!(base < 0 && expect), "4: the call may continue and rebuilds");
            check(base < 3, "the base is no table");
            if (base < 0) rebuild(cur, true); else continued++;
        }
        for (int s = 0; s < c.steps; s++)
            if (!enqueue(c, gtab ? s : -1, tables[s & 1], tables[(s & 1) ^ 1], s == c.fail_step)) return;
        const int final_table = tables[c.steps & 1];
        if (gtab) {
            rot.run_finished(ptr(final_table), c.steps);
            may = true;
            may_q = q;
            may_q.states = ptr(final_table);
        }
        cur = final_table;
    }

    void call(const Call& c) {
        const bool may_now = may;
        const GridQuery may_was = may_q;
        may = false;
        if (c.refill) ver[cur] = next_ver++;
        if (c.steps < 0) solve(c); else run(c, may_now, may_was);
    }
};

}  // namespace

int main() {
    long sequences = 0;
    for (int len = 1; len <= 4; len++) {
        long count = 1;
        for (int i = 0; i < len; i++) count *= LETTERS;
        for (long code = 0; code < count; code++) {
            World w;
            current_sequence.clear();
            long rest = code;
            for (int i = 0; i < len; i++, rest /= LETTERS) {
                const Call& c = ALPHABET[rest % LETTERS];
                current_sequence += (i ? " " : "") + std::string(c.name);
                w.call(c);
            }
            sequences++;
        }
    }
    std::printf("host_state_check: %ld sequences, %ld steps, %ld continued, %ld rebuilt, %ld queue growths, %ld failures\n",
                sequences, steps_run, continued, rebuilt, grown, failures);
    return failures ? 1 : 0;
}
