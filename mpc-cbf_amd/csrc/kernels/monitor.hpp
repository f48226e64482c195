// monitor.hpp — arguments of the closed-loop safety monitor's kernels (monitor.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

struct mpccbf_monitor;

namespace mpccbf {

constexpr int MONITOR_MAX_ROWS = 1 << 20;        // row indices in the first-collision key: 20 bits each
constexpr int64_t MONITOR_MAX_SAMPLES = 1 << 23; // its sample index: 23 bits
constexpr uint64_t MONITOR_NONE = ~0ull;         // no collision yet / not reached yet (-1 as int64)
constexpr uint64_t MONITOR_INF_BITS = 0x7ff0000000000000ull;  // +inf: no row within the watch radius

// summary words (MPCCBF_MONITOR_WORDS of them)
enum { MON_SAMPLES = 0, MON_FIRST_KEY, MON_HITS, MON_UNSAFE, MON_MIN_D2, MON_WORDS };

struct MonitorArgs {
    // the batch: num_samples snapshots of num_states rows
    const double* samples;   // agents' states: sample s, agent a at samples[s * sample_stride + a * row_stride]
    int32_t num_samples;
    int64_t sample_stride, row_stride;
    int32_t agent_first, num_agents;
    const double* fixed;     // num_states x 6, rows outside the agent range (nullptr: there are none)
    int32_t num_states;
    const double* goals;     // num_agents x 3, or nullptr
    int64_t sample_first;    // index of sample 0, or < 0: the samples scored so far (summary[MON_SAMPLES])
    // the tests
    int32_t box;
    double half_x, half_y;   // box: the script's collision_shape; circle: half_x = radius
    double dmin2, goal2, watch2, inv_cell;
    uint32_t mask;           // hash table size - 1
    // outputs
    unsigned long long* summary;
    unsigned long long* reached_at;  // per row, unsigned min of the sample index (MONITOR_NONE: never)
    unsigned long long* min_d2;      // per row, bits of the smallest squared distance
    uint32_t* hit_samples;
    uint32_t* unsafe_samples;
    unsigned long long* sample_log;  // sample_log_rows x 3, or nullptr
    int32_t sample_log_rows;
    // scratch (monitor_carve)
    unsigned long long* base;  // this call's first sample index
    uint32_t* cnt;             // num_samples x T
    uint32_t* start;           // num_samples x (T + 1)
    uint32_t* slot;            // num_samples x 2 x num_states: bucket, offset inside it
    uint32_t* sorted;          // num_samples x num_states
};

uint32_t monitor_table_size(int num_rows);
size_t monitor_scratch_bytes(int num_rows, int num_samples);
void monitor_carve(void* scratch, int num_rows, int num_samples, MonitorArgs& a);

hipError_t launch_monitor_reset(const MonitorArgs& a, int rows, hipStream_t s);
// count memset, insert, scan + scatter, query: four operations on the stream
hipError_t launch_monitor_score(const MonitorArgs& a, hipStream_t s);

// What mpccbf_set_monitor refuses of a monitor's own fields (empty: nothing)
std::string monitor_attach_error(const mpccbf_monitor* m);

// The body of mpccbf_monitor_score (capi_control.hip): every check on the host, then the launches
int monitor_enqueue(const mpccbf_monitor* m, const double* samples, int32_t num_samples, int64_t sample_stride,
                    int64_t row_stride, int32_t agent_first, int32_t num_agents, const double* fixed_states,
                    int32_t num_states, const double* goals, int64_t sample_first, int32_t device, void* stream);

}  // namespace mpccbf
