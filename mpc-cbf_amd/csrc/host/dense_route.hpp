// dense_route.hpp — what the host decides for one mpccbf_qp_solve_dense_batch call, as plain
// C++17 (no HIP header, no library): the limits of the generic dense QP path, the shape of a QP as
// the route sees it, the route itself (slices, each slice's LDS geometry and staging, the PDIP
// instantiation, the active-set launch and its early exit) as functions of the shapes alone, the
// slot reserved for a QP before it is packed, and the byte layout of the three buffers of a call.
// dense_qp.hip follows it; tools/dense_route_check.cpp prints and checks it without a device.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mpccbf {

// ---- limits (host and device code: dense_qp.hip's kernels, dense_pack.hpp, dense_qp.cpp)
constexpr int DENSE_NZ = 8;        // reduced dimension (padded)
constexpr int DENSE_ROWS = 256;    // reduced inequality rows: 64 lanes x 4 slots
constexpr int DENSE_NMAX = 64;     // variables per QP on the device elimination (lane = variable)
constexpr int DENSE_EMAX = 64;     // equalities per QP on the device elimination (lane = equality)
constexpr int DQ_R = DENSE_ROWS / 64;
constexpr int DQ_HDR = 2 * DENSE_NZ * DENSE_NZ + DENSE_NZ + 2;  // P, LP, q, reg, pad
constexpr int DQ_ROW = DENSE_NZ + 2;                            // g, lo, hi
constexpr double kInf = 1e300;     // |bound| >= 1e300 means "absent" (numeric_limits lowest/max)
constexpr double kFeasTol = 1e-6;  // CPLEX default feasibility tolerance (CPLEX.cpp:8 default ctor)
// reduction statuses beyond qpcpp::SolveStatus: -1 = the PDIP solves it; capacity errors
constexpr int RS_SOLVE = -1, RS_CAP_NZ = -2, RS_CAP_ROWS = -3;
// the solver's settings (DenseBatch maxit / das_steps / tol; feas_tol = kFeasTol)
constexpr int kDenseMaxIt = 100;     // PDIP iterations
constexpr int kDenseDasSteps = 48;   // dual active-set steps before the PDIP (0: the PDIP alone)
constexpr double kDenseTol = 1e-9;
// rows the active-set launch takes (the wave PDIP's row capacity, kernels/pdip_wave.hpp WROWS)
constexpr int DENSE_DAS_ROWS = 192;

// zero rows after the E^T image: the QR's row loops run in unguarded chunks of ET_PAD rows (16
// took the kernel to 141 registers, three waves per SIMD, for no gain in the QR)
constexpr int ET_PAD = 8;

// E^T / H image in dynamic LDS, sized per slice: rows = the slice's largest n, row stride S = the
// larger of its largest n and equality count, made odd (spread banks); at most 64 x 65 doubles
constexpr int reduce_stride(int nmax, int emax) { return (nmax > emax ? nmax : emax) | 1; }

namespace dense_route {

constexpr int SLICE_COUNT = 1024;          // count >= SLICE_COUNT: 4 pack / reduce slices, else 1
constexpr int MAX_SLICES = 4;
constexpr int EARLY_COUNT = 64;            // count <= EARLY_COUNT: the early exit's host check
constexpr size_t STAGE_BYTES = 48 * 1024;  // LDS image + staged packed QP at most this, else no staging
constexpr int PACK_SPARE = 1;              // spare word after a packed QP (pack_qp's compaction), staged with it

// ---- the exact sizes of a packed QP (dense_pack.hpp pack_qp) and the slot reserved for it
constexpr size_t packed_doubles(size_t n, size_t nh, size_t me, size_t enz, size_t mi, size_t inz) {
    return n + 1 + nh + me + enz + 2 * mi + inz;
}
// int32 words: header, inequality row pointers, then the u16 / u8 arrays
constexpr size_t packed_ints(size_t nh, size_t me, size_t enz, size_t mi, size_t inz) {
    return 4 + (mi + 1) + (2 * (me + 1) + 2 * nh + enz + inz + 3) / 4;
}

// Sizes reserved for QP (n, m) before it is read: the exact sizes at nh <= n (n + 1) / 2, me and
// mi <= m + n (every row an inequality costs the most doubles) and enz + inz <= m n + n, plus the
// spare word; nred = its reduced-QP block (the reduced rows are a subset of the inequality rows,
// a QP with more than DENSE_ROWS is a capacity error before its rows are read; >= 1 row: the
// kernel reads row 0). A QP that is not packed (an argument error, n > DENSE_NMAX) has no slot.
struct SlotBound {
    size_t nd = 0, ni = 0, nred = 0;
};
inline SlotBound slot_bound(int64_t n, int64_t m) {
    SlotBound b;
    if (n >= 1 && n <= DENSE_NMAX && m >= 0) {
        const size_t hmax = (size_t)(n * (n + 1) / 2), rows = (size_t)(m + n), nzmax = (size_t)(m * n + n);
        b.nd = packed_doubles((size_t)n, hmax, 0, 0, rows, nzmax) + PACK_SPARE;
        b.ni = packed_ints(hmax, rows, 0, rows, nzmax) + PACK_SPARE;
    }
    const int64_t rows_k = (n >= 1 && m >= 0) ? std::min<int64_t>(m + n, DENSE_ROWS) : 1;
    b.nred = (size_t)DQ_HDR + (size_t)std::max<int64_t>(rows_k, 1) * DQ_ROW;
    return b;
}

// ---- one QP as the route sees it
struct QpShape {
    int n = 1, me = 0;
    int rows = 0;           // packed inequality rows; of a host-reduced QP, its reduced rows
    size_t nd = 0, ni = 0;  // packed doubles / ints (exact, without the spare word)
    bool cap = false;       // beyond the device elimination: reduced on the host, not packed
};

// ---- slices: slice i of n is [q0[i], q0[i + 1])
struct Slices {
    int n = 0;
    int q0[MAX_SLICES + 1] = {0, 0, 0, 0, 0};
};
inline Slices slices_of(int count) {
    Slices s;
    const int nslice = count >= SLICE_COUNT ? MAX_SLICES : 1;
    const int step = (count + nslice - 1) / nslice;
    for (int q = 0; q < count; q += step) s.q0[s.n++] = q;
    s.q0[s.n] = count;
    return s;
}

// A slice's reduce launch: sized by its own largest QP; the packed QPs are staged in LDS when the
// image and the largest packed QP fit STAGE_BYTES (beyond: the kernel reads its QP over the bus
// where it uses it). Host-reduced QPs do not count.
struct SliceRoute {
    int lds_rows = 1, lds_stride = 1;
    int stage_d = 0, stage_i = 0;  // staged doubles / ints (0: direct)
    size_t lds_bytes = 0;          // dynamic LDS of the launch
};
inline SliceRoute slice_route(const QpShape* q, int q0, int q1) {
    int nmax = 1, emax = 1;
    size_t sd = 0, si = 0;
    for (int k = q0; k < q1; k++) {
        if (q[k].cap) continue;
        nmax = std::max(nmax, q[k].n);
        emax = std::max(emax, q[k].me);
        sd = std::max(sd, q[k].nd + PACK_SPARE);
        si = std::max(si, q[k].ni + PACK_SPARE);
    }
    SliceRoute r;
    r.lds_rows = nmax;
    r.lds_stride = reduce_stride(nmax, emax);
    r.lds_bytes = (size_t)(r.lds_rows + ET_PAD) * r.lds_stride * sizeof(double);
    const size_t stage = sd * sizeof(double) + si * sizeof(int32_t);
    if (r.lds_bytes + stage <= STAGE_BYTES) {
        r.stage_d = (int)sd;
        r.stage_i = (int)si;
        r.lds_bytes += stage;
    }
    return r;
}

// ---- the call
inline std::vector<int> host_reduced(const QpShape* q, int count) {
    std::vector<int> big;
    for (int k = 0; k < count; k++)
        if (q[k].cap) big.push_back(k);
    return big;
}

// The launches after the reductions. The active-set launch settles most QPs and writes their final
// outputs; a small batch without a host-reduced QP whose QPs it all settled needs no PDIP and no
// expansion launch (early_exit: the host checks the pinned statuses after one synchronisation).
struct CallRoute {
    int rows_max = 1;  // the call's largest row count, capped at DENSE_ROWS
    bool active_set = false;
    int R = 1;  // dense_qp_kernel<DENSE_NZ, R>: row slots per lane
    bool early_exit = false;
};
inline CallRoute call_route(const QpShape* q, int count) {
    CallRoute r;
    bool any_cap = false;
    for (int k = 0; k < count; k++) {
        r.rows_max = std::max(r.rows_max, std::min(q[k].rows, DENSE_ROWS));
        any_cap |= q[k].cap;
    }
    r.active_set = kDenseDasSteps > 0 && r.rows_max <= DENSE_DAS_ROWS;
    r.R = r.rows_max <= 64 ? 1 : (r.rows_max <= 128 ? 2 : DQ_R);
    r.early_exit = r.active_set && count <= EARLY_COUNT && !any_cap;
    return r;
}

// ---- the buffers of a call: every section at a 16-byte boundary of its buffer
struct Section {
    size_t off = 0, bytes = 0;
};
template <class T>
T* section_ptr(void* base, Section s) {
    return (T*)((char*)base + s.off);
}
constexpr size_t align16(size_t v) { return (v + 15) & ~size_t(15); }

struct DenseLayout {
    // pinned input (written by the host, read by the kernels over the bus)
    Section dbl, ints, off_d, off_i, red_off, hostred, psize;
    size_t in_bytes = 0;
    // pinned output (written by the kernels): the last call's x | obj | status
    Section x, obj, status_out;
    size_t out_bytes = 0;
    // device block
    Section red, zx, y, status, m, pd, iters;
    size_t dev_bytes = 0;
};
// count QPs, nd / ni / nred: the slots' totals (doubles, ints, reduced-QP doubles)
inline DenseLayout dense_layout(size_t count, size_t nd, size_t ni, size_t nred) {
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const Section s{at, bytes};
        at += align16(bytes);
        return s;
    };
    const size_t words = count * sizeof(int32_t), offs = (count + 1) * sizeof(int64_t);
    DenseLayout l;
    l.dbl = take(nd * sizeof(double));
    l.ints = take(ni * sizeof(int32_t));
    l.off_d = take(offs);  // per QP, + the total at [count]
    l.off_i = take(offs);
    l.red_off = take(offs);
    l.hostred = take(words);
    l.psize = take(2 * words);
    l.in_bytes = at;
    at = 0;
    l.x = take(count * DENSE_NMAX * sizeof(double));
    l.obj = take(count * sizeof(double));
    l.status_out = take(words);
    l.out_bytes = at;
    at = 0;
    l.red = take(nred * sizeof(double));
    l.zx = take(count * (DENSE_NMAX * DENSE_NZ + DENSE_NMAX) * sizeof(double));  // Z row-major, then xp
    l.y = take(count * DENSE_NZ * sizeof(double));
    l.status = take(words);
    l.m = take(words);
    l.pd = take(words);
    l.iters = take(words);
    l.dev_bytes = at;
    return l;
}

}  // namespace dense_route
}  // namespace mpccbf
