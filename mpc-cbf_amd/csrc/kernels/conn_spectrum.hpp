// conn_spectrum.hpp — a team's weighted Laplacian spectrum on one wavefront: lambda2 and the unit
// Fiedler vector (ConnectivityCBF::getLambda2, ConnectivityCBF.cpp:368-414). Shared by the CBF-only
// connectivity controller (connectivity_control.hip) and the per-team spectrum launch of the
// batched IMPC's connectivity rows (team_spectrum_kernel, impc_conn.hip; the rows themselves:
// conn_rows_dev.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "group.hpp"

namespace mpccbf {
namespace dev {

constexpr int CC_MAX = 16;  // robots per team

struct ConnLds {
    double A[CC_MAX * CC_MAX];  // Laplacian, diagonalised in place
    double V[CC_MAX * CC_MAX];  // eigenvectors (columns)
    double rot[CC_MAX][2];      // (c, s) of the round's rotations
    double pos[CC_MAX][2];
    double l2, ev[CC_MAX];
    int32_t pairs[CC_MAX / 2][2];
};

// lambda2 and the unit Fiedler vector of the team (n <= 16) into L.l2 / L.ev (all lanes).
// EXIT_EXP: the sweeps end when the off-diagonal mass is <= 1e-EXIT_EXP of the total (sums of
// squares). 32 (connectivity_control_kernel): machine precision, which rounding often keeps out of
// reach, so all 30 sweeps run. 26 (team_spectrum_kernel): off-diagonal norm <= 1e-13 of the
// matrix's — the eigenvalue's error is of second order in it (<= 1e-26 ||A||^2 / gap), the
// eigenvector's of first (<= 1e-13 ||A|| / gap) — reached after a few quadratically converging
// sweeps.
template <int EXIT_EXP = 32>
__device__ void team_lambda2(ConnLds& L, int n, double dmax, int lane) {
    static_assert(EXIT_EXP == 32 || EXIT_EXP == 26, "sweep exit: 1e-32 or 1e-26");
    constexpr double exit_rel = EXIT_EXP == 32 ? 1e-32 : 1e-26;
    const double Rs2 = dmax * dmax, sigma = dmax * dmax * dmax * dmax / 0.69314718055994530942;
    for (int e = lane; e < CC_MAX * CC_MAX; e += 64) {
        const int i = e / CC_MAX, j = e % CC_MAX;
        double a = 0.0;
        if (i < n && j < n && i != j) {
            const double dx = L.pos[i][0] - L.pos[j][0], dy = L.pos[i][1] - L.pos[j][1];
            const double d2 = dx * dx + dy * dy;
            a = d2 <= Rs2 ? -(exp((Rs2 - d2) * (Rs2 - d2) / sigma) - 1.0) : 0.0;
        }
        L.A[e] = a;
        L.V[e] = (i == j && i < n) ? 1.0 : 0.0;
    }
    wave_lds_sync();
    if (lane < n) {  // degrees on the diagonal
        double dg = 0.0;
        for (int j = 0; j < n; j++) dg -= L.A[lane * CC_MAX + j];
        L.A[lane * CC_MAX + lane] = dg;
    }
    wave_lds_sync();
    const int m = n + (n & 1);  // round-robin over m slots (slot n is a dummy when n is odd)
    const int np = m / 2;
    for (int sweep = 0; sweep < 30; sweep++) {
        // convergence: off-diagonal mass against the total
        double off = 0.0, tot = 0.0;
        for (int e = lane; e < CC_MAX * CC_MAX; e += 64) {
            const double a = L.A[e] * L.A[e];
            tot += a;
            off += (e / CC_MAX != e % CC_MAX) ? a : 0.0;
        }
        off = grp_sum<64>(off);
        tot = grp_sum<64>(tot);
        if (off <= exit_rel * tot || off == 0.0) break;
        for (int round = 0; round < m - 1; round++) {
            // pairing of this round (circle method: slot 0 fixed, the others rotate)
            if (lane < np) {
                const int k = lane;
                int p = (k == 0) ? 0 : 1 + (round + k - 1) % (m - 1);
                int q = 1 + (round + m - 2 - k) % (m - 1);
                if (p > q) { const int t = p; p = q; q = t; }
                L.pairs[k][0] = p;
                L.pairs[k][1] = q;
                double c = 1.0, s = 0.0;
                if (q < n) {
                    const double apq = L.A[p * CC_MAX + q];
                    if (apq != 0.0) {
                        const double theta = (L.A[q * CC_MAX + q] - L.A[p * CC_MAX + p]) / (2.0 * apq);
                        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                    }
                }
                L.rot[k][0] = c;
                L.rot[k][1] = s;
            }
            wave_lds_sync();
            // A <- A J (columns p, q) and V <- V J
            for (int task = lane; task < np * CC_MAX; task += 64) {
                const int k = task / CC_MAX, r = task % CC_MAX;
                const int p = L.pairs[k][0], q = L.pairs[k][1];
                if (q < n && r < n) {
                    const double c = L.rot[k][0], s = L.rot[k][1];
                    const double ap = L.A[r * CC_MAX + p], aq = L.A[r * CC_MAX + q];
                    L.A[r * CC_MAX + p] = c * ap - s * aq;
                    L.A[r * CC_MAX + q] = s * ap + c * aq;
                    const double vp = L.V[r * CC_MAX + p], vq = L.V[r * CC_MAX + q];
                    L.V[r * CC_MAX + p] = c * vp - s * vq;
                    L.V[r * CC_MAX + q] = s * vp + c * vq;
                }
            }
            wave_lds_sync();
            // A <- J^T A (rows p, q)
            for (int task = lane; task < np * CC_MAX; task += 64) {
                const int k = task / CC_MAX, r = task % CC_MAX;
                const int p = L.pairs[k][0], q = L.pairs[k][1];
                if (q < n && r < n) {
                    const double c = L.rot[k][0], s = L.rot[k][1];
                    const double ap = L.A[p * CC_MAX + r], aq = L.A[q * CC_MAX + r];
                    L.A[p * CC_MAX + r] = c * ap - s * aq;
                    L.A[q * CC_MAX + r] = s * ap + c * aq;
                }
            }
            wave_lds_sync();
        }
    }
    // second smallest eigenvalue (ties: lower index), its unit eigenvector (eigenvec.normalize())
    if (lane == 0) {
        int k0 = 0;
        for (int i = 1; i < n; i++)
            if (L.A[i * CC_MAX + i] < L.A[k0 * CC_MAX + k0]) k0 = i;
        int k1 = -1;
        for (int i = 0; i < n; i++) {
            if (i == k0) continue;
            if (k1 < 0 || L.A[i * CC_MAX + i] < L.A[k1 * CC_MAX + k1]) k1 = i;
        }
        if (k1 < 0) k1 = k0;
        L.l2 = L.A[k1 * CC_MAX + k1];
        double nrm = 0.0;
        for (int i = 0; i < n; i++) nrm += L.V[i * CC_MAX + k1] * L.V[i * CC_MAX + k1];
        nrm = sqrt(nrm);
        for (int i = 0; i < n; i++) L.ev[i] = L.V[i * CC_MAX + k1] / nrm;
    }
    wave_lds_sync();
}

}  // namespace dev
}  // namespace mpccbf
