// launch_plan_grid.cpp — the IMPC launch decisions over a grid of hand-filled operators, as text.
//
// Two builds of one source, so that both walk the same grid:
//   default   — asks impc_launch_plan (csrc/kernels/launch_plan.hpp). Built by the Makefile as
//               build/launch_plan_grid; tests/test_launch_plan.py compares its output with
//               tests/golden/launch_plan_parent.txt.
//   -DPARENT  — asks the selection functions the plan replaced (impc_kernel_name, impc_clock_waves,
//               impc_store_ok, impc_may_defer, impc_rows_may_exceed, impc_conn_*), composed as
//               capi.hip composed them. RUN AT THE PARENT OF THE CHANGE THAT INTRODUCED THE PLAN,
//               linked to that commit's libmpccbf.so; its output is the fixture:
//                 hipcc -x hip --offload-host-only -std=c++17 -DPARENT -Impc-cbf_amd/csrc/kernels \
//                   tools/launch_plan_grid.cpp -Lmpc-cbf_amd/build -lmpccbf -Wl,-rpath,$PWD/mpc-cbf_amd/build
//
// The grid: six base operator sets (separable K = 15, slack with 16 / 32 rows per channel,
// non-separable nz = 6, FoV, FoV slack), each with one selection-relevant field at a time moved
// across every threshold of the selection code, crossed with variant 0..5, agents {0, 5, 1024,
// 1025} (wide_max = 1024), store attached or not, caller lists or grid, knn_k {8, 9}; then with
// connectivity attached at the four agent counts.
// Output: "T <index> <token>" lines (token = name|clock waves|store|defers|8-slot capacity launch,
// the last '-' where no capacity launch follows or slack mode picks it), then one "P <label>
// <codes>" line per point, two hex digits (a token index) per combination.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "impc.hpp"
#ifndef PARENT
#include "launch_plan.hpp"
#endif

namespace mpccbf {
#ifdef PARENT
const char* impc_kernel_name(const DevOps& op, int variant, int n, bool store);
bool impc_store_ok(const DevOps& op, int variant, int n);
int impc_clock_waves(const DevOps& op, int variant, int n);
bool impc_may_defer(const DevOps& op, int variant, bool csr, int knn_k, int n);
bool impc_rows_may_exceed(const DevOps& op, bool csr, int knn_k);
bool impc_conn_ok(const DevOps& op);
const char* impc_conn_kernel_name();
int impc_conn_clock_waves(int n);
#endif
}  // namespace mpccbf
using namespace mpccbf;

static std::string token(const DevOps& d, int variant, int n, bool store, bool csr, int knn, bool conn) {
    const char* name;
    int waves;
    bool st, defer, cap8, conn_ok = true;
#ifdef PARENT
    DevOps op = d;  // (capi.hip's launch_ops: a store attached turns the lean launch off)
    if (store) op.lean = 0;
    if (conn) {
        name = impc_conn_kernel_name();
        waves = impc_conn_clock_waves(n);
        conn_ok = impc_conn_ok(op);
    } else {
        const char* nm = impc_kernel_name(op, variant, n, store);
        name = d.cbf_mode == 1 ? (d.slack_mode ? "impc_fov_kernel<true>" : "impc_fov_kernel<false>") : (nm ? nm : "");
        waves = impc_clock_waves(op, variant, n);
    }
    st = store && !conn && impc_store_ok(op, variant, n);
    defer = !conn && d.cbf_mode != 1 && impc_may_defer(op, variant, csr, knn, n);
    cap8 = impc_rows_may_exceed(op, csr, knn);
#else
    const LaunchPlan p = impc_launch_plan(d, variant, n, csr, knn, store, conn);
    name = p.name;
    waves = p.clock_waves;
    st = p.store;
    defer = p.defer;
    cap8 = p.capacity == IMPC_QUEUE8 || p.capacity == IMPC_QUEUE8_STORE;
    if (conn) conn_ok = p.kernel == IMPC_CONN;
#endif
    char buf[160];
    std::snprintf(buf, sizeof(buf), "%s|%d|%d|%d|%s%s", name, waves, (int)st, (int)defer,
                  (defer && !d.slack_mode) ? (cap8 ? "1" : "0") : "-", conn ? (conn_ok ? "|ok" : "|refused") : "");
    return buf;
}

struct Field {
    const char* name;
    int32_t DevOps::*f;
    std::vector<int> values;
};

int main() {
    auto base = [](int cbf_mode, int slack, int sep, int rpd, int nz, int m) {
        DevOps d;
        std::memset(&d, 0, sizeof(d));
        d.cbf_mode = cbf_mode;
        d.slack_mode = slack;
        d.sep = sep;
        d.nzd = sep ? 2 : 0;
        d.sep_rows_per_dim = rpd;
        d.sep_sb = (rpd + 15) / 16;
        d.nz = nz;
        d.m = m;
        d.cbf_h = 2;
        d.dual_as = 24;
        d.hot = 1500;
        d.wide_max = 1024;
        return d;
    };
    const std::vector<std::pair<const char*, DevOps>> bases = {
        {"sep15", base(0, 0, 1, 16, 30, 48)},   {"slack16", base(0, 1, 1, 16, 30, 48)},
        {"slack32", base(0, 1, 1, 32, 32, 51)}, {"dense6", base(0, 0, 0, 0, 6, 48)},
        {"fov", base(1, 0, 0, 0, 15, 60)},      {"fovslack", base(1, 1, 0, 0, 15, 60)},
    };
    const std::vector<Field> fields = {
        {"sep", &DevOps::sep, {0, 1}},
        {"nzd", &DevOps::nzd, {2, 3}},
        {"rpd", &DevOps::sep_rows_per_dim, {16, 17, 32, 33}},
        {"cbf_h", &DevOps::cbf_h, {2, 3, 8, 9}},
        {"dual_as", &DevOps::dual_as, {0, 24}},
        {"lean", &DevOps::lean, {0, 1}},
        {"hot", &DevOps::hot, {0, 2048, 2049}},
        {"m", &DevOps::m, {63, 64, 192, 193, 255, 256}},
        {"nz", &DevOps::nz, {5, 6, 7, 14, 15, 16}},
    };
    const int counts[] = {0, 5, 1024, 1025};
    std::map<std::string, int> index;
    std::vector<std::string> tokens, lines;
    auto code = [&](const std::string& t) {
        auto it = index.find(t);
        if (it == index.end()) {
            it = index.emplace(t, (int)tokens.size()).first;
            tokens.push_back(t);
        }
        char h[8];
        std::snprintf(h, sizeof(h), "%02x", it->second);
        return std::string(h);
    };
    for (const auto& b : bases)
        for (const Field& f : fields)
            for (int v : f.values) {
                DevOps d = b.second;
                d.*(f.f) = v;
                std::string ln = std::string("P ") + b.first + "/" + f.name + "=" + std::to_string(v) + " ";
                for (int variant = 0; variant <= 5; variant++)
                    for (int n : counts)
                        for (int store = 0; store < 2; store++)
                            for (int csr = 0; csr < 2; csr++)
                                for (int knn = 8; knn <= 9; knn++)
                                    ln += code(token(d, variant, n, store != 0, csr != 0, knn, false));
                for (int n : counts) ln += code(token(d, 0, n, false, false, 8, true));
                lines.push_back(ln);
            }
    if (tokens.size() > 256) {
        std::fprintf(stderr, "more than 256 distinct tokens\n");
        return 1;
    }
    for (size_t i = 0; i < tokens.size(); i++) std::printf("T %02zx %s\n", i, tokens[i].c_str());
    for (const std::string& ln : lines) std::puts(ln.c_str());
    return 0;
}
