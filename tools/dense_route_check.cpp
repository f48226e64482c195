// dense_route_check — the host's decisions for mpccbf_qp_solve_dense_batch without a device
// (csrc/host/dense_route.hpp, the host-reduced block of csrc/host/dense_qp.cpp). Plain C++: no
// HIP, no library.
//
//   dense_route_check < calls     each call: a count, then one line per QP "n me rows nd ni cap";
//                                 prints the limits, then each call's route as one line
//   dense_route_check             (no input) checks the buffers' layout, the slices, the slot bounds
//                                 and the host-reduced block; exits non-zero on any failure
//
// Test driver of tests/test_dense_route_inputs.py.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "dense_pack.hpp"
#include "dense_qp.hpp"
#include "dense_route.hpp"

using namespace mpccbf;
using namespace mpccbf::dense_route;

static int g_failures = 0;
static long g_checks = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        g_checks++;                              \
        if (!(cond)) {                           \
            g_failures++;                        \
            std::printf("FAIL %s: ", #cond);     \
            std::printf(__VA_ARGS__);            \
            std::printf("\n");                   \
        }                                        \
    } while (0)

// ---- routes of the calls on stdin
static void print_limits() {
    std::printf("limits DENSE_NZ=%d DENSE_ROWS=%d DENSE_NMAX=%d DENSE_EMAX=%d ET_PAD=%d DAS_ROWS=%d SLICE_COUNT=%d "
                "MAX_SLICES=%d EARLY_COUNT=%d STAGE_BYTES=%zu PACK_SPARE=%d\n",
                DENSE_NZ, DENSE_ROWS, DENSE_NMAX, DENSE_EMAX, ET_PAD, DENSE_DAS_ROWS, SLICE_COUNT, MAX_SLICES,
                EARLY_COUNT, STAGE_BYTES, PACK_SPARE);
}

static void print_route(const std::vector<QpShape>& q) {
    const int count = (int)q.size();
    const Slices s = slices_of(count);
    std::printf("route slices=");
    for (int i = 0; i < s.n; i++) {
        const SliceRoute r = slice_route(q.data(), s.q0[i], s.q0[i + 1]);
        std::printf("%s%d:%d:%d:%d:%zu:%d:%d", i ? ";" : "", s.q0[i], s.q0[i + 1], r.lds_rows, r.lds_stride, r.lds_bytes,
                    r.stage_d, r.stage_i);
    }
    const CallRoute c = call_route(q.data(), count);
    std::printf(" rows_max=%d active_set=%d R=%d early_exit=%d host_reduced=", c.rows_max, (int)c.active_set, c.R,
                (int)c.early_exit);
    const std::vector<int> big = host_reduced(q.data(), count);
    for (size_t b = 0; b < big.size(); b++) std::printf("%s%d", b ? "," : "", big[b]);
    std::printf("\n");
}

static bool routes_from_stdin() {
    int count;
    if (std::scanf("%d", &count) != 1) return false;
    print_limits();
    do {
        std::vector<QpShape> q(count > 0 ? count : 0);
        for (QpShape& s : q) {
            long long nd, ni;
            int cap;
            if (std::scanf("%d %d %d %lld %lld %d", &s.n, &s.me, &s.rows, &nd, &ni, &cap) != 6) {
                std::printf("FAIL: truncated call\n");
                g_failures++;
                return true;
            }
            s.nd = (size_t)nd;
            s.ni = (size_t)ni;
            s.cap = cap != 0;
        }
        print_route(q);
    } while (std::scanf("%d", &count) == 1);
    return true;
}

// ---- the buffers' layout
static void check_layout(size_t count, size_t nd, size_t ni, size_t nred) {
    const DenseLayout l = dense_layout(count, nd, ni, nred);
    struct Named {
        const char* name;
        int buf;
        Section s;
        size_t need;  // bytes the call uses
    };
    const size_t w = count * sizeof(int32_t), o = (count + 1) * sizeof(int64_t);
    const Named sec[] = {{"dbl", 0, l.dbl, nd * 8}, {"ints", 0, l.ints, ni * 4}, {"off_d", 0, l.off_d, o},
                         {"off_i", 0, l.off_i, o}, {"red_off", 0, l.red_off, count * 8}, {"hostred", 0, l.hostred, w},
                         {"psize", 0, l.psize, 2 * w}, {"x", 1, l.x, count * DENSE_NMAX * 8}, {"obj", 1, l.obj, count * 8},
                         {"status_out", 1, l.status_out, w}, {"red", 2, l.red, nred * 8},
                         {"zx", 2, l.zx, count * (DENSE_NMAX * DENSE_NZ + DENSE_NMAX) * 8}, {"y", 2, l.y, count * DENSE_NZ * 8},
                         {"status", 2, l.status, w}, {"m", 2, l.m, w}, {"pd", 2, l.pd, w}, {"iters", 2, l.iters, w}};
    const size_t total[3] = {l.in_bytes, l.out_bytes, l.dev_bytes};
    const int nsec = (int)(sizeof(sec) / sizeof(sec[0]));
    for (int a = 0; a < nsec; a++) {
        const Named& A = sec[a];
        CHECK(A.s.off % 16 == 0, "%s at %zu (count %zu, nd %zu, ni %zu, nred %zu)", A.name, A.s.off, count, nd, ni, nred);
        CHECK(A.s.bytes >= A.need, "%s holds %zu of %zu bytes (count %zu)", A.name, A.s.bytes, A.need, count);
        CHECK(A.s.off + A.s.bytes <= total[A.buf], "%s ends at %zu of %zu (count %zu)", A.name, A.s.off + A.s.bytes,
              total[A.buf], count);
        for (int b = a + 1; b < nsec; b++) {
            const Named& B = sec[b];
            if (A.buf != B.buf) continue;
            CHECK(A.s.off + A.s.bytes <= B.s.off || B.s.off + B.s.bytes <= A.s.off, "%s and %s overlap (count %zu)", A.name,
                  B.name, count);
        }
    }
}

static void check_slices(int count) {
    const Slices s = slices_of(count);
    CHECK(s.n == (count >= 1024 ? 4 : 1) && s.n <= MAX_SLICES, "count %d: %d slices", count, s.n);
    CHECK(s.q0[0] == 0 && s.q0[s.n] == count, "count %d: covers [%d, %d)", count, s.q0[0], s.q0[s.n]);
    for (int i = 0; i < s.n; i++) CHECK(s.q0[i] < s.q0[i + 1], "count %d: slice %d is empty or out of order", count, i);
}

// ---- the slot reserved before packing against plan_qp's exact sizes, for the densest QP of a
// shape: a full H, every row of A full; all m rows and n variables inequalities (the most
// doubles), or the first min(m, 64) rows equalities (the most row pointers beside them)
static void check_slot_bounds() {
    const int N = DENSE_NMAX, M = 300;
    const std::vector<double> ones((size_t)M * N, 1.0), vlo(N, -1.0), vhi(N, 1.0);
    std::vector<double> lo(M, -1.0), hi(M, 1.0);
    for (int n = 1; n <= N; n++)
        for (int m = 0; m <= M; m++)
            for (int eq = 0; eq <= (n == 1 || n == 8 || n == N ? 1 : 0); eq++) {
                const int me = eq ? std::min(m, DENSE_EMAX) : 0;
                for (int k = 0; k < me; k++) lo[k] = hi[k] = 1.0;
                mpccbf_dense_qp qp{};
                qp.n = n;
                qp.m = m;
                qp.H = qp.c = qp.A = ones.data();
                qp.lo = lo.data();
                qp.hi = hi.data();
                qp.vlo = vlo.data();
                qp.vhi = vhi.data();
                const dense_pack::PackPlan pl = dense_pack::plan_qp(qp);
                for (int k = 0; k < me; k++) lo[k] = -1.0, hi[k] = 1.0;
                const SlotBound b = slot_bound(n, m);
                CHECK(pl.err.empty() && !pl.cap && pl.me == me && pl.mi == m - me + n, "n %d m %d: %s", n, m, pl.err.c_str());
                CHECK(b.nd >= pl.nd + PACK_SPARE, "n %d m %d me %d: %zu doubles reserved, %zu packed", n, m, me, b.nd, pl.nd);
                CHECK(b.ni >= pl.ni + PACK_SPARE, "n %d m %d me %d: %zu ints reserved, %zu packed", n, m, me, b.ni, pl.ni);
                CHECK(b.nred == (size_t)DQ_HDR + (size_t)std::min(pl.mi + pl.me, DENSE_ROWS) * DQ_ROW,
                      "n %d m %d: %zu reduced doubles", n, m, b.nred);
            }
    // no slot for a QP that is not packed; its reduced block still holds a row
    for (const int64_t nm : {0, -1, DENSE_NMAX + 1}) {
        const SlotBound b = slot_bound(nm, 3);
        CHECK(b.nd == 0 && b.ni == 0 && b.nred >= (size_t)DQ_HDR + DQ_ROW, "n %lld: %zu %zu %zu", (long long)nm, b.nd, b.ni,
              b.nred);
    }
    CHECK(slot_bound(4, -1).nd == 0 && slot_bound(4, -1).nred == (size_t)DQ_HDR + DQ_ROW, "m -1");
}

// ---- the host-reduced block, by position
static void check_block(const char* name, const ReducedQP& r, double ridge) {
    const ReducedBlock b = device_block(r);
    const int NZ = DENSE_NZ;
    CHECK(b.status == RS_SOLVE && b.m == r.m && b.pd == (r.pd ? 1 : 0), "%s: words %d %d %d", name, b.status, b.m, b.pd);
    CHECK(b.dbl.size() == (size_t)DQ_HDR + (size_t)r.m * DQ_ROW, "%s: %zu doubles", name, b.dbl.size());
    if (b.dbl.size() != (size_t)DQ_HDR + (size_t)r.m * DQ_ROW) return;
    for (int i = 0; i < NZ; i++)
        for (int j = 0; j < NZ; j++) {
            const bool in = i < r.nz && j < r.nz;
            const double eye = i == j ? 1.0 : 0.0;
            CHECK(b.dbl[i * NZ + j] == (in ? r.P(i, j) : eye), "%s: P(%d, %d) = %g", name, i, j, b.dbl[i * NZ + j]);
            const double lp = (in && r.pd) ? (j <= i ? r.LP(i, j) : 0.0) : eye;
            CHECK(b.dbl[NZ * NZ + i * NZ + j] == lp, "%s: LP(%d, %d) = %g", name, i, j, b.dbl[NZ * NZ + i * NZ + j]);
        }
    for (int i = 0; i < NZ; i++)
        CHECK(b.dbl[2 * NZ * NZ + i] == (i < r.nz ? r.q[i] : 0.0), "%s: q[%d] = %g", name, i, b.dbl[2 * NZ * NZ + i]);
    CHECK(b.dbl[2 * NZ * NZ + NZ] == ridge, "%s: ridge %g, expected %g", name, b.dbl[2 * NZ * NZ + NZ], ridge);
    CHECK(b.dbl[2 * NZ * NZ + NZ + 1] == 0.0, "%s: pad", name);
    for (int k = 0; k < r.m; k++) {
        const double* row = &b.dbl[DQ_HDR + (size_t)k * DQ_ROW];
        for (int j = 0; j < NZ; j++) CHECK(row[j] == (j < r.nz ? r.G(k, j) : 0.0), "%s: g(%d, %d) = %g", name, k, j, row[j]);
        CHECK(row[NZ] == r.lo[k] && row[NZ + 1] == r.hi[k], "%s: bounds of row %d", name, k);
    }
}

static void check_blocks() {
    ReducedQP pd;  // positive definite, nz = 3, m = 2
    pd.n = 5;
    pd.nz = 3;
    pd.m = 2;
    pd.pd = true;
    pd.P = Mat(3, 3);
    pd.LP = Mat(3, 3);
    const double L[3][3] = {{2.0, 0.0, 0.0}, {0.5, 1.5, 0.0}, {-1.0, 0.25, 3.0}};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            pd.LP(i, j) = L[i][j];
            for (int k = 0; k < 3; k++) pd.P(i, j) += L[i][k] * L[j][k];
        }
    pd.q = {0.5, -1.5, 2.5};
    pd.G = Mat(2, 3);
    for (int k = 0; k < 2; k++)
        for (int j = 0; j < 3; j++) pd.G(k, j) = 10.0 * (k + 1) + j + 0.25;
    pd.lo = {-3.0, -kInf};
    pd.hi = {kInf, 7.0};
    check_block("positive definite", pd, 0.0);

    ReducedQP sd;  // semidefinite (no factor), nz = 2, m = 1: the ridge scales with |P|max
    sd.n = 4;
    sd.nz = 2;
    sd.m = 1;
    sd.pd = false;
    sd.P = Mat(2, 2);
    sd.P(0, 0) = 4.0;
    sd.P(0, 1) = sd.P(1, 0) = -2.0;
    sd.P(1, 1) = 1.0;
    sd.q = {1.0, -1.0};
    sd.G = Mat(1, 2);
    sd.G(0, 0) = 1.0;
    sd.G(0, 1) = -2.0;
    sd.lo = {-1.0};
    sd.hi = {1.0};
    check_block("semidefinite", sd, 1e-10 * 4.0);
    sd.P(0, 0) = 0.5;  // |P|max below 1: the ridge's floor
    sd.P(0, 1) = sd.P(1, 0) = 0.0;
    sd.P(1, 1) = 0.0;
    check_block("semidefinite, small", sd, 1e-10);

    // the decision's order: inconsistent equalities, capacity nz, capacity rows, a violated constant row
    ReducedQP d;
    d.eq_infeasible = true;
    d.status = MPCCBF_INFEASIBLE;
    d.nz = DENSE_NZ + 1;
    d.m = DENSE_ROWS + 44;
    ReducedBlock b = device_block(d);
    CHECK(b.status == MPCCBF_INFEASIBLE && b.m == DENSE_ROWS, "inconsistent equalities first: %d %d", b.status, b.m);
    CHECK(b.dbl.size() == (size_t)DQ_HDR + (size_t)DENSE_ROWS * DQ_ROW, "decided block: %zu doubles", b.dbl.size());
    for (const double v : b.dbl) CHECK(v == 0.0, "decided block holds %g", v);
    d.eq_infeasible = false;  // (status INFEASIBLE: a violated constant row)
    CHECK(device_block(d).status == RS_CAP_NZ, "capacity nz before rows: %d", device_block(d).status);
    d.nz = DENSE_NZ;
    CHECK(device_block(d).status == RS_CAP_ROWS, "capacity rows before a constant row: %d", device_block(d).status);
    d.m = 0;
    CHECK(device_block(d).status == MPCCBF_INFEASIBLE, "a violated constant row: %d", device_block(d).status);
    d.status = MPCCBF_OPTIMAL;
    d.nz = 0;
    CHECK(device_block(d).status == MPCCBF_OPTIMAL, "nz = 0 decided: %d", device_block(d).status);
}

int main() {
    if (!routes_from_stdin()) {
        const size_t counts[] = {1, 2, 63, 64, 65, 1023, 1024, 1027, 4096};
        for (const size_t count : counts) {
            check_slices((int)count);
            // no packed QP at all, odd word counts, the bench's QP (36 variables, 94 rows), the largest slots
            const SlotBound big = slot_bound(DENSE_NMAX, 300);
            const SlotBound mid = slot_bound(36, 94);
            check_layout(count, 0, 0, count * (size_t)(DQ_HDR + DQ_ROW));
            check_layout(count, 3 * count + 1, 5 * count + 3, count * (size_t)(DQ_HDR + DQ_ROW) + 1);
            check_layout(count, count * mid.nd, count * mid.ni, count * mid.nred);
            check_layout(count, count * big.nd + 7, count * big.ni + 1, count * big.nred);
        }
        check_slot_bounds();
        check_blocks();
        std::printf("dense_route_check: %ld checks, %d failures\n", g_checks, g_failures);
    }
    return g_failures ? 1 : 0;
}
