// active_store.hpp — the active-set store (mpccbf_set_active_store): per agent one record of 8
// int32 [k | 5 side keys | steps | IMPC iteration] that a step writes and the next step reads.
// Keys name a side independently of lanes and slots, so a record survives a change of slot, of
// neighbour order and of kernel layout:
//   box side  -> (channel * 16 + row) * 2 + upper          (0 .. 95)
//   CBF side  -> -(1 + neighbour's state index * 8 + sample) (< 0)
// Reading maps keys onto this QP's own sides by comparison only (no address is formed from a
// key): a box key must be in range and name a row the operators have; a CBF key must name a
// neighbour that has a staged row (tags, one key per staged CBF row, written by the staging).
// Iteration 0 has the sample-0 rows only, so every sample of neighbour j maps to j's one row there.
// A set that does not fit the solver's factor (k > KMAX) starts cold.
#pragma once

#include <stdint.h>

#include "group.hpp"
#include "impc.hpp"
#include "impc_wide.hpp"
#include "pdip_sep.hpp"

namespace mpccbf {
namespace dev {

constexpr int AS_KEYS = 5;                   // side keys a record holds (DK of the 16-lane solver)
constexpr int AS_BOX_KEYS = 2 * SEP_D * 16;  // box keys are 0 .. AS_BOX_KEYS - 1
static_assert(DK <= AS_KEYS, "a record holds the 16-lane solver's whole active set");

// neighbour of a CBF key (key < 0; INT_MIN included: no overflow). Every sample of the neighbour
// maps: an A/B build measured same-sample-only and next-sample-only keys
__device__ __forceinline__ int as_key_nb(int key) { return (int)((unsigned)(-(key + 1)) >> 3); }

// The record's keys as side ids of the 16-lane layout (pdip_sep.hpp POL_ID: side * 16 + lane; box
// side 2 d + upper of lane = row, CBF slot c of lane l = staged row c * 16 + l) into ids[0 .. n);
// returns n (0: cold start). rec / tags: LDS by type (the record's 8 words; the staged rows' keys).
// Group-uniform: every lane computes the same n, lane 0 writes.
template <int CB>
__device__ __forceinline__ int as_map_sep(lds_vptr<int32_t> rec, lds_vptr<int32_t> tags, int count, int rows_per_dim,
                                          int min_steps, int gl, double* ids) {
    const int kr = rec[0];
    if (min_steps < 0 || kr <= 0 || kr > DK || rec[6] < min_steps) return 0;
    const int live = count < CB * 16 ? count : CB * 16;
    int got[DK], n = 0;
#pragma unroll
    for (int i = 0; i < DK; i++) got[i] = -1;
#pragma unroll
    for (int i = 0; i < DK; i++) {
        if (i >= kr) continue;
        const int key = rec[1 + i];
        int id = -1;
        if (key >= 0) {
            const int row = (key >> 1) & 15;
            if (key < AS_BOX_KEYS && row < rows_per_dim) id = (2 * (key >> 5) + (key & 1)) * 16 + row;
        } else {  // (a CBF key: every sample of the neighbour maps)
            const int nb = as_key_nb(key);
#pragma unroll
            for (int c = 0; c < CB; c++) {
                const int slot = c * 16 + gl;
                const bool hit = slot < live && as_key_nb(tags[slot < live ? slot : 0]) == nb;
                const unsigned m = (unsigned)grp_ballot<16>(hit);
                if (m != 0u && id < 0) id = (2 * SEP_D + c) * 16 + (__ffs(m) - 1);
            }
        }
        // (a box row's other side too: both sides of a row are dependent, never both active)
        bool dup = id < 0;
#pragma unroll
        for (int j = 0; j < DK; j++) dup = dup || got[j] == id || (key >= 0 && got[j] == (id ^ 16));
        if (dup) continue;
#pragma unroll
        for (int j = 0; j < DK; j++) got[j] = j == n ? id : got[j];
        if (gl == 0) ids[n] = (double)id;
        n++;
    }
    return n;
}

// This lane's word of the record of a solve's final set (lane w < 8 forms word w): ids[0 .. k)
// the 16-lane side ids, k = ids[POL_K] (< 0: the optimum has no exact active set, zero record).
__device__ __forceinline__ int as_word_sep(const double* ids, lds_vptr<int32_t> tags, int steps, int it, int gl) {
    const int k = (int)ids[POL_K];
    if (k < 0 || k > AS_KEYS || gl >= AS_WORDS) return 0;
    if (gl == 0) return k;
    if (gl == 6) return steps;
    if (gl == 7) return it;
    if (gl - 1 >= k) return 0;
    const int id = (int)ids[gl - 1], s = id >> 4, ln = id & 15;
    if (s < 2 * SEP_D) return (((s >> 1) * 16 + ln) << 1) | (s & 1);
    return tags[(s - 2 * SEP_D) * 16 + ln];
}

// The same for the one-agent-per-wave layout (impc_wide.hpp: side id = lane * 2 + upper, box lane
// = channel * 16 + row — a box key is its side id — and CBF lane W_BOX + staged row). A record of
// more than WK sides (written by the 16-lane layout) starts cold.
__device__ __forceinline__ int as_map_wide(lds_vptr<int32_t> rec, lds_vptr<int32_t> tags, int count, int rows_per_dim,
                                           int min_steps, int gl, double* ids) {
    const int kr = rec[0];
    if (min_steps < 0 || kr <= 0 || kr > WK || rec[6] < min_steps) return 0;
    const int live = count < W_CBF ? count : W_CBF;
    int got[WK], n = 0;
#pragma unroll
    for (int i = 0; i < WK; i++) got[i] = -1;
#pragma unroll
    for (int i = 0; i < WK; i++) {
        if (i >= kr) continue;
        const int key = rec[1 + i];
        int id = -1;
        if (key >= 0) {
            if (key < AS_BOX_KEYS && ((key >> 1) & 15) < rows_per_dim) id = key;
        } else {  // (a CBF key: every sample of the neighbour maps)
            const int nb = as_key_nb(key);
            const bool hit = gl < live && as_key_nb(tags[gl < live ? gl : 0]) == nb;
            const unsigned long long m = __ballot(hit);
            if (m != 0ull) id = (W_BOX + (__ffsll((long long)m) - 1)) * 2 + 1;
        }
        bool dup = id < 0;
#pragma unroll
        for (int j = 0; j < WK; j++) dup = dup || got[j] == id || (key >= 0 && got[j] == (id ^ 1));
        if (dup) continue;
#pragma unroll
        for (int j = 0; j < WK; j++) got[j] = j == n ? id : got[j];
        if (gl == 0) ids[n] = (double)id;
        n++;
    }
    return n;
}

__device__ __forceinline__ int as_word_wide(const double* ids, lds_vptr<int32_t> tags, int steps, int it, int gl) {
    const int k = (int)ids[POL_K];
    if (k < 0 || k > AS_KEYS || gl >= AS_WORDS) return 0;
    if (gl == 0) return k;
    if (gl == 6) return steps;
    if (gl == 7) return it;
    if (gl - 1 >= k) return 0;
    const int id = (int)ids[gl - 1];
    if (id < AS_BOX_KEYS) return id;
    return tags[(id >> 1) - W_BOX];
}

}  // namespace dev
}  // namespace mpccbf
