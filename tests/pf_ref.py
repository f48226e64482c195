"""numpy restatement of the batched FoV particle filter (mpccbf_pf_init / mpccbf_pf_step,
csrc/kernels/pf_fov.hip): pf::ParticleFilter (particle_filter.cpp) driven by
PFApplications::processFovUpdate (pf_applications.cpp:6-44), with the product's counter-based draws
(csrc/kernels/pf_stream.hpp) in place of the reference's unseeded std::mt19937.

Besides the results, step() returns per pair the decision margin: how far the step's discrete
decisions (inside / outside the field of view, which ancestor a resampling draw picks) are from
flipping. The device and this file differ only through libm's last bits and the order of sums of
<= 1024 terms (~1e-13); a case whose margins stay above 1e-10 takes the same decisions in both."""
import numpy as np

COMP_X, COMP_Y, COMP_RESAMPLE, COMP_INIT_X, COMP_INIT_Y = range(5)
FLAG_MEASURED, FLAG_DEGENERATE = 1, 2


def params(fov, Rs, num_particles=100, init_cov=(1.0, 0.0, 1.0), process=(0.25, 0.0, 0.0, 0.25),
           meas_cov=(0.05, 0.0, 0.05), dt=0.2, weight_reduction=10.0, seed=0):
    """The fields of mpccbf_pf_params (defaults: CBFControl_example.cpp:96-99, dt 0.2, reduction 10)."""
    return dict(num_particles=int(num_particles), init_cov=tuple(init_cov), process=tuple(process),
                meas_cov=tuple(meas_cov), dt=float(dt), fov=float(fov), Rs=float(Rs),
                weight_reduction=float(weight_reduction), seed=int(seed))


def _u64(v):
    return np.asarray(v, dtype=np.int64).astype(np.uint64)


def mix64(z):
    """splitmix64's mixer on uint64 arrays (pf_mix64)."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def keys(seed, step, observer, neighbour, num_particles, comp):
    """The keys of one pair's particles for one component (pf_pair_key, pf_key)."""
    k = mix64(np.array([seed & ((1 << 64) - 1)], dtype=np.uint64))
    for word in (step, observer, neighbour):
        k = mix64(k ^ _u64([word]))
    with np.errstate(over="ignore"):
        return mix64(k ^ (np.arange(num_particles, dtype=np.uint64) * np.uint64(8) + np.uint64(comp)))


def uniform(key):
    return (key >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _cospi(x):
    """cos(pi x) for x in [0, 2) with an exact argument reduction (the device's cospi)."""
    n = np.rint(2.0 * x)
    r = x - 0.5 * n  # exact, |r| <= 1/4
    q = n.astype(np.int64) % 4
    c, s = np.cos(np.pi * r), np.sin(np.pi * r)
    return np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))


def normal(key):
    """Box-Muller (pf_normal): u1 in (0, 1] from the key, u2 in [0, 1) from the key mixed once more."""
    u1 = ((key >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = uniform(mix64(key))
    return np.sqrt(-2.0 * np.log(u1)) * _cospi(2.0 * u2)


def fov_frame(ego, px, py):
    """math::insideFOV's quantities (Geometry.cpp:59-73): (|bearing|, distance) in the ego frame."""
    c, s = np.cos(ego[2]), np.sin(ego[2])
    dx, dy = px - ego[0], py - ego[1]
    lx, ly = c * dx + s * dy, -s * dx + c * dy
    return np.abs(np.arctan2(ly, lx)), np.sqrt(lx * lx + ly * ly)


def _pairs(agent_first, rp, col):
    for i in range(len(rp) - 1):
        for e in range(int(rp[i]), int(rp[i + 1])):
            yield e, agent_first + i, int(col[e])


def chol(cov3):
    l00 = np.sqrt(cov3[0])
    l10 = cov3[1] / l00
    return l00, l10, np.sqrt(cov3[2] - l10 * l10)


def init(par, states, agent_first, rp, col, init_xy=None, step_index=0, out=None):
    """ParticleFilter::init per pair (particle_filter.cpp:12-56). Arrays are indexed by the CSR entry
    (rp[-1] rows; rows before rp[0] are left as `out` has them, zero without `out`)."""
    P, n = par["num_particles"], int(rp[-1])
    r = out or dict(particles=np.zeros((n, 2, P)), weights=np.zeros((n, P)), est_xy=np.zeros((n, 2)),
                    est_cov=np.zeros((n, 3)), flags=np.zeros(n, dtype=np.int32))
    l00, l10, l11 = chol(par["init_cov"])
    for e, obs, nb in _pairs(agent_first, rp, col):
        x0 = np.asarray(states[nb][:2] if init_xy is None else init_xy[e], dtype=np.float64)
        z0 = normal(keys(par["seed"], step_index, obs, nb, P, COMP_INIT_X))
        z1 = normal(keys(par["seed"], step_index, obs, nb, P, COMP_INIT_Y))
        r["particles"][e, 0] = x0[0] + l00 * z0
        r["particles"][e, 1] = x0[1] + (l10 * z0 + l11 * z1)
        r["weights"][e] = 1.0 / P
        r["est_xy"][e] = x0
        r["est_cov"][e] = par["init_cov"]
        r["flags"][e] = 0
    return r


def step(par, states, agent_first, rp, col, particles, weights, step_index, input=None):
    """processFovUpdate per pair from the given particles / weights (not modified). Returns a dict of
    arrays indexed by the CSR entry: particles, weights (after resampling), predicted and
    pre_weights (what resampling gathered from), ancestors, flags, est_xy, est_cov and margin (inf
    for rows outside rp[0] .. rp[-1])."""
    P, n = par["num_particles"], int(rp[-1])
    W, R = par["process"], par["meas_cov"]
    det = R[0] * R[2] - R[1] * R[1]
    ixx, ixy, iyy = R[2] / det, -R[1] / det, R[0] / det
    half = 0.5 * par["fov"]
    r = dict(particles=np.array(particles, dtype=np.float64), weights=np.array(weights, dtype=np.float64),
             predicted=np.zeros((n, 2, P)), pre_weights=np.zeros((n, P)),
             ancestors=np.zeros((n, P), dtype=np.int32), flags=np.zeros(n, dtype=np.int32),
             est_xy=np.zeros((n, 2)), est_cov=np.zeros((n, 3)), margin=np.full(n, np.inf))
    for e, obs, nb in _pairs(agent_first, rp, col):
        ego, tgt = states[obs], states[nb]
        ux, uy = (0.0, 0.0) if input is None else input[e]
        # predict (particle_filter.cpp:63-75)
        z0 = normal(keys(par["seed"], step_index, obs, nb, P, COMP_X))
        z1 = normal(keys(par["seed"], step_index, obs, nb, P, COMP_Y))
        x = (particles[e, 0] + ux * par["dt"]) + (W[0] * z0 + W[1] * z1)
        y = (particles[e, 1] + uy * par["dt"]) + (W[2] * z0 + W[3] * z1)
        # negative information (pf_applications.cpp:19-26)
        ang, dist = fov_frame(ego, x, y)
        inside = (ang <= half) & (dist <= par["Rs"])
        w = np.where(inside, weights[e] / par["weight_reduction"], weights[e])
        s2 = w.sum()
        degenerate = not (s2 > 0.0 and np.isfinite(s2))
        # measurement update of a visible neighbour (pf_applications.cpp:29-33, particle_filter.cpp:85-100)
        tang, tdist = fov_frame(ego, tgt[0], tgt[1])
        measured = bool(tang <= half and tdist <= par["Rs"])
        margin = min(np.min(np.abs(ang - half)), np.min(np.abs(dist - par["Rs"])), abs(tang - half),
                     abs(tdist - par["Rs"]))
        make_uniform = degenerate and not measured
        if measured:
            dx, dy = x - tgt[0], y - tgt[1]
            with np.errstate(under="ignore"):
                w = np.exp(-0.5 * (ixx * dx * dx + 2.0 * ixy * dx * dy + iyy * dy * dy))
            s3 = w.sum()
            if s3 > 0.0 and np.isfinite(s3):
                w = w / s3
            else:
                degenerate = make_uniform = True
        if make_uniform:
            w = np.full(P, 1.0 / P)
        # multinomial resampling (particle_filter.cpp:106-118; std::discrete_distribution)
        cum = np.cumsum(w)
        cum = cum / cum[-1]
        u = uniform(keys(par["seed"], step_index, obs, nb, P, COMP_RESAMPLE))
        anc = np.minimum(np.searchsorted(cum, u, side="right"), P - 1)
        upper = np.where(anc < P - 1, np.abs(u - cum[anc]), np.inf)  # (the last particle takes the clamp)
        lower = np.where(anc > 0, np.abs(u - cum[np.maximum(anc - 1, 0)]), np.inf)
        margin = min(margin, upper.min(), lower.min())
        nx, ny = x[anc], y[anc]
        # estimate (particle_filter.cpp:120-124, 153-171)
        mx, my = nx.mean(), ny.mean()
        ddx, ddy = nx - mx, ny - my
        r["predicted"][e, 0], r["predicted"][e, 1], r["pre_weights"][e] = x, y, w
        r["particles"][e, 0], r["particles"][e, 1], r["weights"][e] = nx, ny, w[anc]
        r["ancestors"][e] = anc
        r["flags"][e] = (FLAG_MEASURED if measured else 0) | (FLAG_DEGENERATE if degenerate else 0)
        r["est_xy"][e] = (mx, my)
        r["est_cov"][e] = (np.sum(ddx * ddx) / (P - 1), np.sum(ddx * ddy) / (P - 1), np.sum(ddy * ddy) / (P - 1))
        r["margin"][e] = margin
    return r
