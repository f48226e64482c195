"""Inputs of the FoV IMPC on per-observer neighbour estimates (Context.set_fov_estimates), shared by
tests/test_fov_estimate_inputs.py (CPU: every input pinned against the oracle) and
tests/test_gpu_fov_estimates.py (GPU: the kernel's estimate form against the same oracle values).

Every case stays at the base FoV configuration (fov_beta 120 deg, Ds 0.2, Rs 6). The reference is
the unchanged oracle: for observer a, a copy of the state table whose listed neighbours' (x, y) are
overwritten with the pair's estimate, and a covariance table whose row nb_col[e] is the pair's
covariance (oracle_reference) — valid because the FoV rows use only the neighbour's position."""
import functools
import math

import numpy as np

import oracle_lib as O
from mpccbf import swarm

NO_SLACK = {}
SLACK = dict(slack_mode=1, slack_cost=1000.0, slack_decay_rate=0.9)  # the example's setting
SLACK_ORDER = dict(slack_mode=1, slack_cost=1000.0, slack_decay_rate=0.1)
SETTINGS = {"plain": NO_SLACK, "slack": SLACK}
SIGMA = 0.2  # the swarm cases' estimate error (m)


def config(setting):
    over = SETTINGS[setting] if isinstance(setting, str) else setting
    return swarm.fov_config(20, **over)


def reference_tables(states, lst, nb_xy, nb_cov):
    """The oracle's inputs for one observer: (state table, covariance table or None)."""
    table = np.array(states, dtype=np.float64)
    covs = None if nb_cov is None else np.tile([0.1, 0.0, 0.1], (len(table), 1)).astype(np.float64)
    for e, j in enumerate(lst):
        table[j, :2] = nb_xy[e]
        if covs is not None:
            covs[j] = nb_cov[e]
    return table, covs


def oracle_reference(cfg, states, a, lst, nb_xy, nb_cov, ref):
    """Observer a's IMPC on its own estimates: nb_xy / nb_cov are the rows of its pairs, in list order."""
    table, covs = reference_tables(states, lst, nb_xy, nb_cov)
    # (slack mode with unknown covariances: the oracle's covs=None is every distance -5)
    return O.impc_optimize(O.make_params(cfg), table, a, np.asarray(lst, dtype=np.int32), ref, covs=covs)


def oracle_batch(cfg, case, nb_cov="case"):
    """Every observer of a case on the oracle: (status (agents x impc_iter), obj)."""
    cov = case["nb_cov"] if isinstance(nb_cov, str) else nb_cov
    rp, col, first = case["rp"], case["col"], case["agent_first"]
    st, ob = [], []
    for i in range(case["num_agents"]):
        sl = slice(rp[i], rp[i + 1])
        r = oracle_reference(cfg, case["states"], first + i, col[sl], case["nb_xy"][sl],
                             None if cov is None else cov[sl], case["refs"][i])
        st.append(r["status"])
        ob.append(r["obj"])
    return np.array(st), np.array(ob)


def random_spd(rng, pairs, lo=0.02, hi=0.3):
    """Covariances (cxx, cxy, cyy) with variances in [lo, hi] and |correlation| <= 0.8."""
    var = rng.uniform(lo, hi, size=(pairs, 2))
    rho = rng.uniform(-0.8, 0.8, size=pairs)
    return np.stack([var[:, 0], rho * np.sqrt(var[:, 0] * var[:, 1]), var[:, 1]], axis=1)


@functools.lru_cache(maxsize=None)
def swarm_case(n):
    """heading_swarm(n) with the 8 nearest visible neighbours; estimates = the true position +
    SIGMA N(0, I), covariances random SPD, drawn in this order from default_rng(7)."""
    states, targets = swarm.heading_swarm(n)
    rp, col = swarm.fov_csr(states, 8, 6.0, 2.0 * math.pi / 3.0)
    rng = np.random.default_rng(7)
    pairs = int(rp[-1])
    nb_xy = states[col, :2] + SIGMA * rng.normal(size=(pairs, 2))
    nb_cov = random_spd(rng, pairs)
    return dict(states=states, targets=targets, refs=swarm.refs_from_targets(targets, 20), rp=rp, col=col,
                nb_xy=nb_xy, nb_cov=nb_cov, agent_first=0, num_agents=n, cov_table=np.tile([0.1, 0.0, 0.1], (n, 1)))


def fan(k, target=(2.0, 0.3), centre=(0.0, 0.0), seed=11):
    """One observer at `centre`, yaw 0, velocity (0.3, 0), and k static neighbours at bearings spread
    over +-45 deg and ranges 2.6 .. 5.0 m; estimates 0.15 m off the true positions in seeded
    directions. Returns (observer state, target, neighbour states (k x 6), estimates (k x 2))."""
    obs = np.array([centre[0], centre[1], 0.0, 0.3, 0.0, 0.0])
    bear = np.deg2rad(np.linspace(-45.0, 45.0, k)) if k > 1 else np.zeros(1)
    rng_ = np.linspace(2.6, 5.0, k) if k > 1 else np.array([2.6])
    nbs = np.zeros((k, 6))
    nbs[:, 0] = centre[0] + rng_ * np.cos(bear)
    nbs[:, 1] = centre[1] + rng_ * np.sin(bear)
    ang = np.random.default_rng(seed + k).uniform(-math.pi, math.pi, k)
    est = nbs[:, :2] + 0.15 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    tg = np.array([centre[0] + target[0], centre[1] + target[1], 0.0])
    return obs, tg, nbs, est


def fan_case(ks, lead_pairs=0, lead_rows=0, spacing=40.0):
    """Fans of ks neighbours in one batch: the table holds lead_rows unrelated rows, every fan's
    neighbours, then the observers (agent_first > 0); the lists start at pair lead_pairs
    (nb_row_ptr[0] > 0, unrelated rows ahead in the pair buffers). Fan f is centred at (spacing f, 0)."""
    obs, tgs, nbs, ests, lists = [], [], [], [], []
    row = lead_rows
    for f, k in enumerate(ks):
        o, tg, nb, est = fan(k, centre=(spacing * f, 0.0))
        obs.append(o)
        tgs.append(tg)
        nbs.append(nb)
        ests.append(est)
        lists.append(np.arange(row, row + k, dtype=np.int32))
        row += k
    lead = np.zeros((lead_rows, 6))
    lead[:, 0] = -100.0 - 10.0 * np.arange(lead_rows)
    states = np.concatenate([lead] + nbs + [np.array(obs)])
    rp = (lead_pairs + np.concatenate([[0], np.cumsum(ks)])).astype(np.int32)
    col = np.concatenate([np.zeros(lead_pairs, np.int32)] + lists).astype(np.int32)
    nb_xy = np.concatenate([np.full((lead_pairs, 2), 1.0e3)] + ests)
    rng = np.random.default_rng(23)
    nb_cov = random_spd(rng, len(nb_xy))
    targets = np.array(tgs)
    return dict(states=states, targets=targets, refs=swarm.refs_from_targets(targets, 20), rp=rp, col=col,
                nb_xy=nb_xy, nb_cov=nb_cov, agent_first=row, num_agents=len(ks),
                cov_table=np.tile([0.1, 0.0, 0.1], (len(states), 1)))


# fans the oracle solves to OPTIMAL (pinned below), the batches of the GPU test, and the caps
FAN_KS = {"plain": (1, 2, 3, 8, 9, 16), "slack": (1, 2, 3, 8)}
FAN_BATCHES = {"plain": ((3, 16, 9), (1,)), "slack": ((2, 8, 3), (1,))}
FAN_OVER_CAP = {"plain": 17, "slack": 9}


def slack_order_case():
    """Two neighbours at +-78 deg, ranges 3.0 and 3.2, true estimates; covariances A = (0.02 I,
    0.6 I) and B swapped: the slack order, hence the weights, follows the pair's covariance."""
    obs = np.array([0.0, 0.0, 0.0, 0.3, 0.0, 0.0])
    b = math.radians(78.0)
    nbs = np.zeros((2, 6))
    nbs[0, :2] = [3.0 * math.cos(b), 3.0 * math.sin(b)]
    nbs[1, :2] = [3.2 * math.cos(-b), 3.2 * math.sin(-b)]
    states = np.concatenate([nbs, obs[None]])
    targets = np.array([[2.0, 0.0, 0.0]])
    small, large = [0.02, 0.0, 0.02], [0.6, 0.0, 0.6]
    base = dict(states=states, targets=targets, refs=swarm.refs_from_targets(targets, 20),
                rp=np.array([0, 2], np.int32), col=np.array([0, 1], np.int32), nb_xy=nbs[:, :2].copy(),
                agent_first=2, num_agents=1, cov_table=np.tile([0.1, 0.0, 0.1], (3, 1)))
    return {"A": dict(base, nb_cov=np.array([small, large])), "B": dict(base, nb_cov=np.array([large, small]))}


# ---- recorded oracle results (tests/test_fov_estimate_inputs.py holds the oracle to them) --------
# per observer: status and objective of each IMPC iteration (oracle_batch of the case; the key names
# the case and the slack setting)
PINS = {'swarm17/plain': {'status': [[0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0],
                              [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0]],
                   'obj': [[-206.53347743542642, -206.53347743542642], [-358.19829521601645, -358.19829521601645],
                           [-60.90567059559598, -60.90567059559598], [-208.50206431936442, -208.29921854422082],
                           [-145.23718506670207, -145.23718506670207], [-86.08814528586727, -86.08814528586727],
                           [-327.23912685709485, -325.21322454116097], [-282.57193309156776, -281.7831974139045],
                           [-254.83331063685975, -253.79052545671343], [-302.4818434123406, -302.4818434123406],
                           [-155.62638201055464, -155.62638201055464], [-285.54724254623903, -285.54724254623903],
                           [-231.85164616621876, -231.85164616621876], [-80.91623744876377, -80.91623744876377],
                           [-270.5318645022315, -270.5318645022315], [-325.9837179539207, -325.9837179539207],
                           [-340.99337219822564, -340.29371761884556]]},
 'swarm17/slack': {'status': [[0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0],
                              [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0]],
                   'obj': [[-206.53347743542642, -206.53347743542642], [-358.19829521601645, -358.19829521601645],
                           [-60.90567059559598, -60.90567059559598], [-208.50206431939543, -208.29921854080715],
                           [-145.23718506670207, -145.23718506670207], [-86.08814528586727, -86.08814528586727],
                           [-327.23912685742795, -325.21322454248195], [-282.57193308502, -281.7831974178468],
                           [-254.83331063859504, -253.79052545161875], [-302.4818434123406, -302.4818434123406],
                           [-155.62638201055464, -155.62638201055464], [-285.54724254623903, -285.54724254623903],
                           [-231.85164616621876, -231.85164616621876], [-80.91623744876377, -80.91623744876377],
                           [-270.5318645022315, -270.5318645022315], [-325.9837179539207, -325.9837179539207],
                           [-340.99337219685, -340.293717621796]]},
 'swarm33/plain': {'status': [[0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0],
                              [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0],
                              [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0],
                              [0, 0]],
                   'obj': [[-133.7448023073867, -133.7448023073867], [-187.86407249977927, -187.86407249977927],
                           [-94.48743322781837, -94.48743322781837], [-328.4953495704523, -326.49288199896677],
                           [-342.8066770098805, -342.8066770098805], [-172.95939086670674, -172.95939086670674],
                           [-351.65093197037277, -351.65093197037277], [-89.26686119736651, -88.78349091446769],
                           [-230.45883859238285, -229.89035572954597], [-353.07767197073076, -353.07767197073076],
                           [-339.3616263272516, -339.3616263272516], [-253.34271003697307, -253.34271003650588],
                           [-280.7541886883193, -280.7541886883193], [-289.00327781315576, -289.00327781315576],
                           [-201.79081884019604, -201.79081884019604], [-56.652962982087125, -56.652962982087125],
                           [-255.72724533198075, -254.42511258996896], [-100.18927976787353, -100.18927976787353],
                           [-223.18314654836865, -223.18314654836865], [-86.69239764957975, -86.28826647636174],
                           [-63.518612131867094, -63.518612131867094], [-202.99895790101908, -202.99895790101908],
                           [-108.04838211086481, -108.04838211086481], [-364.5434588732816, -363.9271751015853],
                           [-76.63497252994514, -76.42666312903705], [-142.79123226882126, -142.79123226882126],
                           [-260.6089970353, -260.6089970353], [-187.1172992570602, -187.1172992570602],
                           [-318.36664540945713, -318.36664540945713], [-249.44897868874662, -249.44897868874662],
                           [-135.43179915159584, -135.26558495043344], [-250.30644107139415, -250.30644107139415],
                           [-98.6603339615629, -98.6603339615629]]},
 'swarm33/slack': {'status': [[0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0],
                              [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0],
                              [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0],
                              [0, 0]],
                   'obj': [[-133.7448023073867, -133.7448023073867], [-187.86407249977927, -187.86407249977927],
                           [-94.48743322781837, -94.48743322781837], [-328.4953495816585, -326.4928819944215],
                           [-342.8066770098805, -342.8066770098805], [-172.95939086670674, -172.95939086670674],
                           [-351.65093197037277, -351.65093197037277], [-89.26686119870175, -88.78349091612725],
                           [-230.45883859772462, -229.89035573330034], [-353.07767197073076, -353.07767197073076],
                           [-339.3616263272516, -339.3616263272516], [-253.342710011761, -253.34271001885352],
                           [-280.7541886883193, -280.7541886883193], [-289.00327781315576, -289.00327781315576],
                           [-201.79081884019604, -201.79081884019604], [-56.652962982087125, -56.652962982087125],
                           [-255.72724536053974, -254.425112598675], [-100.18927976787353, -100.18927976787353],
                           [-223.18314654836865, -223.18314654836865], [-86.69239765728794, -86.28826647286958],
                           [-63.518612131867094, -63.518612131867094], [-202.99895790101908, -202.99895790101908],
                           [-108.04838211086481, -108.04838211086481], [-364.5434589065092, -363.92717509099134],
                           [-76.63497252784985, -76.42666314214374], [-142.79123226882126, -142.79123226882126],
                           [-260.6089970353, -260.6089970353], [-187.1172992570602, -187.1172992570602],
                           [-318.36664540945713, -318.36664540945713], [-249.44897868874662, -249.44897868874662],
                           [-135.43179913705592, -135.26558494897375], [-250.30644107139415, -250.30644107139415],
                           [-98.6603339615629, -98.6603339615629]]},
 'fan1/plain': {'status': [[0, 0]], 'obj': [[-131.0751192243766, -131.0751192243766]]},
 'fan2/plain': {'status': [[0, 0]], 'obj': [[-121.16696182822322, -117.9421701626375]]},
 'fan3/plain': {'status': [[0, 0]], 'obj': [[-120.04827975478909, -116.79728490072986]]},
 'fan8/plain': {'status': [[0, 0]], 'obj': [[-118.93335733252343, -116.69063339702652]]},
 'fan9/plain': {'status': [[0, 0]], 'obj': [[-123.43030761580344, -120.85741569237813]]},
 'fan16/plain': {'status': [[0, 0]], 'obj': [[-114.63528418719928, -112.62471524285222]]},
 'fans3-16-9/plain': {'status': [[0, 0], [0, 0], [0, 0]],
                      'obj': [[-120.04827975478909, -116.79728490072986], [-114.63528410064913, -112.62471519613506],
                              [-123.43030723723531, -120.857415614542]]},
 'fans1/plain': {'status': [[0, 0]], 'obj': [[-131.0751192243766, -131.0751192243766]]},
 'fan1/slack': {'status': [[0, 0]], 'obj': [[-131.0751192243766, -131.0751192243766]]},
 'fan2/slack': {'status': [[0, 0]], 'obj': [[-121.16696182831878, -117.94217016259658]]},
 'fan3/slack': {'status': [[0, 0]], 'obj': [[-120.04827975474481, -116.79728490076998]]},
 'fan8/slack': {'status': [[0, 0]], 'obj': [[-118.93335733257358, -116.69063339701775]]},
 'fans2-8-3/slack': {'status': [[0, 0], [0, 0], [0, 0]],
                     'obj': [[-121.16696182831878, -117.94217016259658], [-118.93335718689755, -116.6906333068224],
                             [-120.04827937706212, -116.79728470845825]]},
 'fans1/slack': {'status': [[0, 0]], 'obj': [[-131.0751192243766, -131.0751192243766]]},
 'order/A': {'status': [[0, 0]], 'obj': [[32653.1869084949, 58086.83170807491]]},
 'order/B': {'status': [[0, 0]], 'obj': [[7276.423917168784, 14946.377532048842]]},
 'order/none': {'status': [[0, 0]], 'obj': [[7276.423917168784, 14946.377532048842]]}}
