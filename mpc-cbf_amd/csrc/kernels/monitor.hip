// monitor.hip — the closed-loop safety monitor: a batch of S samples (snapshots of N rows' planar
// positions) scored on the stream with the semantics of the reference's post-processing script
// (workspace/experiments/python/metrics/collision_check.py:11-80): colliding pairs, the first
// collision in the script's order, goal arrivals, and the CBF's own margin (pairs inside d_min,
// smallest squared distance).
//
// One spatial hash per sample in the count -> scan -> scatter form of neighbors.hip (cell edge
// grid_inv_cell(watch_radius), table size hash_table_size(N)): a cell holds any number of rows.
// Four operations per batch: the count memset, insert (one thread per sample and row), scan +
// scatter (one block per sample), query (one thread per sample and row over its 3 x 3 cells).
//
// Every accumulated output is an integer: counts by atomic add, minima by 64-bit unsigned atomic
// min — a non-negative double orders as its bit pattern, the first collision is the smallest key
// (sample << 40) | (i << 20) | j — so results do not depend on the order of arrival. The summary
// and the sample log are reduced per wave and per block first: one atomic per block and word.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "impc.hpp"
#include "monitor.hpp"

namespace mpccbf {
namespace dev {

constexpr int MON_BLOCK = 256;
constexpr int MON_SCAN_BLOCK = 1024;

// planar position of row r in sample s; false: the batch has no such row (outside the agent range
// with no table of fixed rows)
__device__ __forceinline__ bool mon_position(const MonitorArgs& a, int s, int r, double& x, double& y) {
    const int ag = r - a.agent_first;
    const double* p;
    if (ag >= 0 && ag < a.num_agents) {
        p = a.samples + (long long)s * a.sample_stride + (long long)ag * a.row_stride;
    } else {
        if (!a.fixed) return false;
        p = a.fixed + (size_t)r * 6;
    }
    x = p[0];
    y = p[1];
    return true;
}

// dx * dx + dy * dy in two roundings of the products and one of the sum, as the host computes it
// (no contraction into a fused multiply-add: the pragma, since the _rn intrinsics are plain
// operators to the compiler and contract like them)
__device__ __forceinline__ double mon_d2(double dx, double dy) {
#pragma clang fp contract(off)
    const double xx = dx * dx, yy = dy * dy;
    return xx + yy;
}

// rectangles_collide (collision_check.py:11-20) on the boxes of collision_check (:28-39): corner =
// centre - half / 2, extent = 2 half, for A = the row of the smaller index
__device__ __forceinline__ bool mon_boxes_collide(double x1, double y1, double x2, double y2, double cx, double cy) {
#pragma clang fp contract(off)
    const double xA = x1 - cx / 2, yA = y1 - cy / 2, xB = x2 - cx / 2, yB = y2 - cy / 2;
    const double w = 2 * cx, h = 2 * cy;
    return xA < xB + w && xA + w > xB && yA < yB + h && yA + h > yB;
}

__global__ void __launch_bounds__(MON_BLOCK) monitor_reset_kernel(MonitorArgs a, int rows) {
    const int i = blockIdx.x * MON_BLOCK + threadIdx.x;
    if (i < rows) {
        a.reached_at[i] = MONITOR_NONE;
        a.min_d2[i] = MONITOR_INF_BITS;
        a.hit_samples[i] = 0u;
        a.unsafe_samples[i] = 0u;
    }
    if (a.sample_log && i < a.sample_log_rows) {
        a.sample_log[(size_t)i * 3] = 0ull;
        a.sample_log[(size_t)i * 3 + 1] = 0ull;
        a.sample_log[(size_t)i * 3 + 2] = MONITOR_INF_BITS;
    }
    if (i == 0) {
        a.summary[MON_SAMPLES] = 0ull;
        a.summary[MON_FIRST_KEY] = MONITOR_NONE;
        a.summary[MON_HITS] = 0ull;
        a.summary[MON_UNSAFE] = 0ull;
        a.summary[MON_MIN_D2] = MONITOR_INF_BITS;
    }
}

// one thread per (sample, row): the row's bucket and its offset inside it. Thread 0 also fixes the
// batch's first sample index and counts its samples (the samples past the key's 23 bits are not
// scored and not counted).
__global__ void __launch_bounds__(MON_BLOCK) monitor_insert_kernel(MonitorArgs a, int blocks_per_sample) {
    const int s = blockIdx.x / blocks_per_sample;
    const int i = (blockIdx.x % blocks_per_sample) * MON_BLOCK + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long b0 = a.sample_first >= 0 ? (unsigned long long)a.sample_first : a.summary[MON_SAMPLES];
        const unsigned long long room = b0 < (unsigned long long)MONITOR_MAX_SAMPLES
                                            ? (unsigned long long)MONITOR_MAX_SAMPLES - b0 : 0ull;
        *a.base = b0;
        a.summary[MON_SAMPLES] += room < (unsigned long long)a.num_samples ? room : (unsigned long long)a.num_samples;
    }
    if (i >= a.num_states) return;
    const int n = a.num_states;
    uint32_t* slot = a.slot + (size_t)s * 2 * n;
    double x, y;
    if (!mon_position(a, s, i, x, y)) {
        slot[i] = 0xffffffffu;  // no such row: in no bucket
        return;
    }
    const uint32_t h = cell_hash((long long)floor(x * a.inv_cell), (long long)floor(y * a.inv_cell), a.mask);
    slot[i] = h;
    slot[n + i] = atomicAdd(&a.cnt[(size_t)s * (a.mask + 1u) + h], 1u);
}

// one block per sample: exclusive scan of its bucket counts, then its rows into bucket order
__global__ void __launch_bounds__(MON_SCAN_BLOCK) monitor_scan_scatter_kernel(MonitorArgs a) {
    __shared__ uint32_t part[MON_SCAN_BLOCK];
    const int s = blockIdx.x, t = threadIdx.x, n = a.num_states;
    const int T = (int)(a.mask + 1u);
    const uint32_t* cnt = a.cnt + (size_t)s * T;
    uint32_t* start = a.start + (size_t)s * (T + 1);
    const int per = (T + MON_SCAN_BLOCK - 1) / MON_SCAN_BLOCK;
    const int b = min(t * per, T), e = min(b + per, T);
    uint32_t sum = 0;
    for (int i = b; i < e; i++) sum += cnt[i];
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < MON_SCAN_BLOCK; o <<= 1) {
        const uint32_t v = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = t > 0 ? part[t - 1] : 0u;
    for (int i = b; i < e; i++) {
        start[i] = run;
        run += cnt[i];
    }
    if (t == MON_SCAN_BLOCK - 1) start[T] = part[MON_SCAN_BLOCK - 1];
    __syncthreads();  // (the block's own global stores are visible to it after the barrier)
    const uint32_t* slot = a.slot + (size_t)s * 2 * n;
    uint32_t* sorted = a.sorted + (size_t)s * n;
    for (int i = t; i < n; i += MON_SCAN_BLOCK) {
        const uint32_t h = slot[i];
        if (h != 0xffffffffu) sorted[start[h] + slot[n + i]] = (uint32_t)i;
    }
}

__device__ __forceinline__ unsigned long long mon_wave_min(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t mon_wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one thread per (sample, row); a block lies inside one sample
__global__ void __launch_bounds__(MON_BLOCK) monitor_query_kernel(MonitorArgs a, int blocks_per_sample) {
    __shared__ unsigned long long w_min[MON_BLOCK / 64], w_key[MON_BLOCK / 64];
    __shared__ uint32_t w_hits[MON_BLOCK / 64], w_unsafe[MON_BLOCK / 64];
    const int s = blockIdx.x / blocks_per_sample;
    const int i = (blockIdx.x % blocks_per_sample) * MON_BLOCK + threadIdx.x;
    const int n = a.num_states;
    const unsigned long long sidx = *a.base + (unsigned long long)s;
    if (sidx >= (unsigned long long)MONITOR_MAX_SAMPLES) return;  // (the whole block)
    unsigned long long best = MONITOR_INF_BITS, key = MONITOR_NONE;
    uint32_t hits = 0, unsafe = 0;
    double px = 0.0, py = 0.0;
    if (i < n && mon_position(a, s, i, px, py)) {
        const int T = (int)(a.mask + 1u);
        const uint32_t* start = a.start + (size_t)s * (T + 1);
        const uint32_t* sorted = a.sorted + (size_t)s * n;
        const long long cx = (long long)floor(px * a.inv_cell), cy = (long long)floor(py * a.inv_cell);
        bool row_hit = false, row_unsafe = false;
        for (int c = 0; c < 9; c++) {
            const uint32_t h = cell_hash(cx + (c % 3) - 1, cy + (c / 3) - 1, a.mask);
            // skip a bucket already visited by an earlier cell of this 3x3 block
            bool dup = false;
            for (int p = 0; p < c; p++)
                if (cell_hash(cx + (p % 3) - 1, cy + (p / 3) - 1, a.mask) == h) dup = true;
            if (dup) continue;
            const uint32_t e1 = start[h + 1];
            for (uint32_t e = start[h]; e < e1; e++) {
                const int j = (int)sorted[e];
                if (j == i) continue;
                double qx, qy;
                mon_position(a, s, j, qx, qy);  // (a row in a bucket exists)
                const double d2 = mon_d2(qx - px, qy - py);
                if (!(d2 <= a.watch2)) continue;
                const unsigned long long bits = (unsigned long long)__double_as_longlong(d2);
                best = bits < best ? bits : best;
                const bool lower = i < j;
                const bool inside = d2 < a.dmin2;
                bool hit;
                if (a.box)
                    hit = lower ? mon_boxes_collide(px, py, qx, qy, a.half_x, a.half_y)
                                : mon_boxes_collide(qx, qy, px, py, a.half_x, a.half_y);
                else
                    hit = d2 <= (2 * a.half_x) * (2 * a.half_x);
                row_hit = row_hit || hit;
                row_unsafe = row_unsafe || inside;
                if (lower && inside) unsafe++;
                if (lower && hit) {
                    hits++;
                    const unsigned long long k = (sidx << 40) | ((unsigned long long)i << 20) | (unsigned long long)j;
                    key = k < key ? k : key;
                }
            }
        }
        // the row's own words: at most one atomic per word, only where it changes something
        if (best != MONITOR_INF_BITS) atomicMin(&a.min_d2[i], best);
        if (row_hit) atomicAdd(&a.hit_samples[i], 1u);
        if (row_unsafe) atomicAdd(&a.unsafe_samples[i], 1u);
        const int ag = i - a.agent_first;
        if (a.goals && ag >= 0 && ag < a.num_agents) {
            const double gx = px - a.goals[(size_t)ag * 3], gy = py - a.goals[(size_t)ag * 3 + 1];
            if (mon_d2(gx, gy) <= a.goal2) atomicMin(&a.reached_at[i], sidx);
        }
    }
    // per wave, per block, then one atomic per block and word
    best = mon_wave_min(best);
    key = mon_wave_min(key);
    hits = mon_wave_sum(hits);
    unsafe = mon_wave_sum(unsafe);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        w_min[w] = best;
        w_key[w] = key;
        w_hits[w] = hits;
        w_unsafe[w] = unsafe;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < MON_BLOCK / 64; k++) {
        best = w_min[k] < best ? w_min[k] : best;
        key = w_key[k] < key ? w_key[k] : key;
        hits += w_hits[k];
        unsafe += w_unsafe[k];
    }
    if (hits) atomicAdd(&a.summary[MON_HITS], (unsigned long long)hits);
    if (unsafe) atomicAdd(&a.summary[MON_UNSAFE], (unsigned long long)unsafe);
    if (key != MONITOR_NONE) atomicMin(&a.summary[MON_FIRST_KEY], key);
    if (best != MONITOR_INF_BITS) atomicMin(&a.summary[MON_MIN_D2], best);
    if (a.sample_log && sidx < (unsigned long long)a.sample_log_rows) {
        unsigned long long* row = a.sample_log + (size_t)sidx * 3;
        if (hits) atomicAdd(&row[0], (unsigned long long)hits);
        if (unsafe) atomicAdd(&row[1], (unsigned long long)unsafe);
        if (best != MONITOR_INF_BITS) atomicMin(&row[2], best);
    }
}

}  // namespace dev

// neighbors.hip's rule: a power of two >= 2 n (>= 1024)
uint32_t monitor_table_size(int num_rows) {
    uint32_t T = 1024;
    while (T < 2u * (uint32_t)num_rows) T <<= 1;
    return T;
}

static inline size_t mon_al256(size_t v) { return (v + 255) & ~(size_t)255; }

// header (the batch's first sample index) | counts | starts | bucket + offset | rows in bucket order
size_t monitor_scratch_bytes(int num_rows, int num_samples) {
    const size_t T = monitor_table_size(num_rows), n = (size_t)num_rows, S = (size_t)num_samples;
    return 256 + mon_al256(S * T * 4) + mon_al256(S * (T + 1) * 4) + mon_al256(S * 2 * n * 4) + mon_al256(S * n * 4);
}

void monitor_carve(void* scratch, int num_rows, int num_samples, MonitorArgs& a) {
    const size_t T = monitor_table_size(num_rows), n = (size_t)num_rows, S = (size_t)num_samples;
    char* p = (char*)scratch;
    a.base = (unsigned long long*)p;
    p += 256;
    a.cnt = (uint32_t*)p;
    p += mon_al256(S * T * 4);
    a.start = (uint32_t*)p;
    p += mon_al256(S * (T + 1) * 4);
    a.slot = (uint32_t*)p;
    p += mon_al256(S * 2 * n * 4);
    a.sorted = (uint32_t*)p;
}

hipError_t launch_monitor_reset(const MonitorArgs& a, int rows, hipStream_t s) {
    const int m = rows > a.sample_log_rows ? rows : a.sample_log_rows;
    const int blocks = m > 0 ? (m + dev::MON_BLOCK - 1) / dev::MON_BLOCK : 1;
    hipLaunchKernelGGL(dev::monitor_reset_kernel, dim3(blocks), dim3(dev::MON_BLOCK), 0, s, a, rows);
    return hipGetLastError();
}

hipError_t launch_monitor_score(const MonitorArgs& a, hipStream_t s) {
    const size_t T = (size_t)a.mask + 1;
    hipError_t e = hipMemsetAsync(a.cnt, 0, (size_t)a.num_samples * T * 4, s);
    if (e != hipSuccess) return e;
    const int bps = (a.num_states + dev::MON_BLOCK - 1) / dev::MON_BLOCK;
    const unsigned blocks = (unsigned)bps * (unsigned)a.num_samples;
    hipLaunchKernelGGL(dev::monitor_insert_kernel, dim3(blocks), dim3(dev::MON_BLOCK), 0, s, a, bps);
    hipLaunchKernelGGL(dev::monitor_scan_scatter_kernel, dim3(a.num_samples), dim3(dev::MON_SCAN_BLOCK), 0, s, a);
    hipLaunchKernelGGL(dev::monitor_query_kernel, dim3(blocks), dim3(dev::MON_BLOCK), 0, s, a, bps);
    return hipGetLastError();
}

}  // namespace mpccbf
