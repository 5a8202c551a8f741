"""fp64 restatement of the rollout decision (etp_nav_decide, include/etpnav_hip.h; vlnce_baselines/ss_trainer_ETP.py:880-977) that the
tests of csrc/decide.hip and etpnav_amd/decide.py compare against, the conditions those comparisons rest on, the bound of stop_prob
and the rollout driver the fixture generator (tools/make_golden_decide.py), the CPU tests and the GPU test share.

episode_ref restates steps 1-6 for one episode in numpy fp64 on the arrays of graph_inputs.pack_episode:
  1. p = softmax(logits) (-inf -> exactly 0), stop_prob = p[0];  2. greedy = lowest index among equal maxima of the logits;
  3. sampled = first index whose inclusive prefix sum of p exceeds u0 * total, clamped to the last p > 0; the teacher label if
     u1 <= sample_ratio;  4. row[cur] = stop_prob, stop_node = lowest index among equal maxima of row[:n];
  5. stop if action == 0 or force_stop or m == 0, else ghost = action - 1 - n and its nearest front (first minimum in list order);
  6. the shortest path cur -> target (Dijkstra) without its first node.

Bound of stop_prob (stop_prob_bound; no multiplier).  The kernel computes e_k = expf(l_k - max) (expf: <= 1 ulp, HIP math API; the
subtraction is rounded once: relative u |l_k - max| in e_k), sums the e_k over a tree whose longest addition chain is SUM_CHAIN = 10
for any G <= 512 (<= 2 entries per thread, a 64-lane butterfly, four wave sums) and divides once.  With r_k = u |l_k - max| + 2u
(u = 2^-24): |stop_prob - p_0| <= p_0 (r_0 + sum_k p_k r_k + (SUM_CHAIN + 1) u) + 2^-126 (flush to zero).

check_conditions asserts, on this restatement alone, what makes the discrete outputs of an fp32 implementation well defined:
  * no alternative predecessor of any node is within MARGIN = 1e-4 (relative to the longest shortest-path distance) of the node's
    distance: the path is unique (fp32 path sums err by at most 64 * 2^-24 relative);
  * the second-nearest front of the chosen ghost is farther by the same margin -- or exactly as far with integer coordinates, where
    fp32 and fp64 both compute the tie exactly (the crafted tie);
  * u0 is at least 4 G 2^-23 away from every cdf boundary below the last positive entry (crossing a later one is absorbed by the
    clamp to the last p > 0);
  * the stop score written in this call differs from the maximum of the row's other entries by more than 10 x its bound -- or the
    logit row is one-hot, where p_0 is exactly 1 or 0 in any precision.
"""
import json

import numpy as np

from etpnav_amd.graph_inputs import pack_batch, pack_episode

U32 = 2.0 ** -24
EXPF_REL = 2.0 * U32          # expf: <= 1 ulp
SUM_CHAIN = 10
FTZ = 2.0 ** -126
MARGIN = 1e-4
IGNORE = -100
STOP, ERR_ACTION, ERR_UNREACHABLE, ERR_INPUT = 1, 2, 4, 8
MUTATIONS = ("argmax_last", "mix_lt", "stop_last", "front_last", "path_first", "keep_ghost", "no_force_stop", "wrong_slot")
WORST = {}
INF = float("inf")


# ---- one episode ----------------------------------------------------------------------------------------------------------------------
def softmax64(l):
    l = np.asarray(l, dtype=np.float64)
    e = np.where(np.isneginf(l), 0.0, np.exp(l - l.max()))
    return e / e.sum()


def dijkstra(adj, src):
    """adj [n,n] fp64 (< 0: no edge) -> (dist, parent) from src"""
    n = len(adj)
    dist, par, done = np.full(n, INF), np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=bool)
    dist[src] = 0.0
    for _ in range(n):
        v = int(np.where(done, INF, dist).argmin())
        if done[v] or not np.isfinite(dist[v]):
            break
        done[v] = True
        for j in range(n):
            if j != v and adj[v, j] >= 0 and dist[v] + adj[v, j] < dist[j]:
                dist[j], par[j] = dist[v] + adj[v, j], v
    return dist, par


def episode_ref(ep, logits, row, u=None, teacher=None, sample_ratio=0.0, force_stop=False, mut=None):
    """ep: pack_episode dict; logits [G]; row [64]: the episode's stop-score row BEFORE the call; u: (u0, u1) or None -> dict"""
    n, m, cur = int(ep["n_nodes"]), int(ep["n_ghost"]), int(ep["cur_node"])
    l = np.asarray(logits, dtype=np.float64)
    p = softmax64(l)
    stop_prob = float(p[0])
    ties = np.nonzero(l == l.max())[0]
    greedy = int(ties[-1] if mut == "argmax_last" else ties[0])
    action, sampled = greedy, None
    if u is not None:
        cdf = np.cumsum(p)
        last = int(np.nonzero(p > 0)[0][-1])
        sampled = min(int(np.searchsorted(cdf, float(u[0]) * cdf[-1], side="right")), last)
        ratio = float(np.float32(sample_ratio))
        take = teacher is not None and (float(u[1]) < ratio if mut == "mix_lt" else float(u[1]) <= ratio)
        action = int(teacher) if take else sampled
    row = np.array(row, dtype=np.float64)
    row[cur] = stop_prob
    st = np.nonzero(row[:n] == row[:n].max())[0]
    stop_node = int(st[-1] if mut == "stop_last" else st[0])
    stop = action == 0 or (force_stop and mut != "no_force_stop") or m == 0
    flags, ghost, target, fdist = (STOP if stop else 0), -1, (stop_node if stop else -1), None
    if not stop:
        if not 1 + n <= action < 1 + n + m:
            flags |= ERR_ACTION
        else:
            ghost = action - 1 - n
            fronts = ep["ghost_fronts"][ghost]
            fdist = np.array([np.sqrt(((ep["node_pos"][f] - ep["ghost_pos"][ghost]) ** 2).sum()) for f in fronts])
            eq = np.nonzero(fdist == fdist.min())[0]
            target = int(fronts[eq[-1] if mut == "front_last" else eq[0]])
    dist, par = dijkstra(np.asarray(ep["adj"], dtype=np.float64), cur)
    path = []
    if target >= 0:
        if not np.isfinite(dist[target]):
            flags |= ERR_UNREACHABLE
        else:
            k = target
            while k != cur:
                path.append(int(k))
                k = par[k]
            path = path[::-1]
            if mut == "path_first":
                path = [cur] + path
    return dict(action=int(action), greedy=greedy, flags=flags, stop_node=stop_node, target=target, ghost=ghost, path=path,
                stop_prob=stop_prob, row=row, p=p, sampled=sampled, dist=dist, par=par, fdist=fdist)


def stop_prob_bound(logits):
    l = np.asarray(logits, dtype=np.float64)
    p = softmax64(l)
    t = np.where(np.isfinite(l), np.abs(l - l.max()), 0.0)          # a -inf logit gives an exact 0
    r = U32 * t + EXPF_REL
    return float(p[0] * (r[0] + (p * r).sum() + (SUM_CHAIN + 1) * U32) + FTZ)


def check_conditions(ep, logits, row, u=None, teacher=None, sample_ratio=0.0, force_stop=False, name=""):
    """assert the module docstring's four conditions on the fp64 restatement -> episode_ref's result"""
    r = episode_ref(ep, logits, row, u, teacher, sample_ratio, force_stop)
    n, cur = int(ep["n_nodes"]), int(ep["cur_node"])
    adj = np.asarray(ep["adj"], dtype=np.float64)
    dist, par = r["dist"], r["par"]
    scale = max(float(dist[np.isfinite(dist)].max()), 1e-30)
    for v in range(n):
        if v == cur or not np.isfinite(dist[v]):
            continue
        for i in range(n):
            if i != v and i != par[v] and adj[i, v] >= 0 and np.isfinite(dist[i]):
                gap = dist[i] + adj[i, v] - dist[v]
                assert gap >= MARGIN * scale, f"{name}: node {v} has predecessor {i} within {gap / scale:.3g} of its shortest path"
    if r["fdist"] is not None and len(r["fdist"]) > 1:
        d = np.sort(r["fdist"])
        g = int(r["ghost"])
        integer = bool((ep["node_pos"] == np.round(ep["node_pos"])).all() and (ep["ghost_pos"][g] == np.round(ep["ghost_pos"][g])).all())
        assert d[1] - d[0] >= MARGIN * max(scale, d[0]) or (d[1] == d[0] and integer), \
            f"{name}: the two nearest fronts of ghost {g} are {d[1] - d[0]:.3g} apart"
    l = np.asarray(logits, dtype=np.float64)
    if u is not None:
        cdf = np.cumsum(r["p"]) / r["p"].sum()
        last = int(np.nonzero(r["p"] > 0)[0][-1])
        if last > 0:
            gap = float(np.abs(cdf[:last] - float(u[0])).min())
            assert gap >= 4 * len(l) * 2.0 ** -23, f"{name}: u0 sits {gap:.3g} from a cdf boundary"
    others = np.array(row, dtype=np.float64)[:n].copy()
    others[cur] = -INF
    if n > 1 and np.isfinite(others.max()):
        sep = abs(r["stop_prob"] - float(others.max()))
        assert int(np.isfinite(l).sum()) == 1 or sep > 10 * stop_prob_bound(l), \
            f"{name}: the written stop score is {sep:.3g} from the row's other maximum (bound {stop_prob_bound(l):.3g})"
    return r


def record(key, got, ref, E, name=""):
    """|got - ref| <= E (no multiplier); the worst ratio goes to WORST[key]"""
    assert np.isfinite(got), f"{name}: non-finite stop_prob"
    ratio = abs(float(got) - float(ref)) / E
    if ratio > WORST.get(key, (0.0, ""))[0]:
        WORST[key] = (ratio, name)
    assert ratio <= 1.0, f"{name}: |got - ref| = {ratio:.3g} x the bound (got {got:.9g}, ref {ref:.9g}, bound {E:.3g})"
    return ratio


def record_row(r, Nmax):
    """the int32 record etp_nav_decide writes for episode_ref's result (stop_prob bits left 0)"""
    out = np.full(8 + Nmax, -1, dtype=np.int64)
    out[:7] = [r["action"], r["greedy"], r["flags"], r["stop_node"], r["target"], r["ghost"], len(r["path"])]
    out[7] = 0
    out[8:8 + len(r["path"])] = r["path"]
    return out


# ---- operator cases the GPU test runs ---------------------------------------------------------------------------------------------------
def random_episode(n, m, rng, cur=None):
    """a walk of n nodes in the xz-plane (steps of 1.5 .. 3), its chain edges plus ~15 % extra ones (Euclidean lengths), m ghosts
    with 1 .. 3 fronts each near one of them"""
    pos = np.zeros((n, 3))
    for i in range(1, n):
        a, d = rng.uniform(0, 2 * np.pi), rng.uniform(1.5, 3.0)
        pos[i] = pos[i - 1] + [d * np.sin(a), rng.uniform(-0.1, 0.1), d * np.cos(a)]
    adj = np.full((n, n), -1.0)
    for i in range(n):
        for j in range(i + 1, n):
            if j == i + 1 or rng.random() < 0.15 * min(1.0, 8.0 / n):
                adj[i, j] = adj[j, i] = np.sqrt(((pos[i] - pos[j]) ** 2).sum())
    fronts = [[int(f) for f in rng.choice(n, size=int(min(n, rng.integers(1, 4))), replace=False)] for _ in range(m)]
    gpos = np.array([pos[f[0]] + rng.uniform(-2.0, 2.0, 3) * [1, 0.05, 1] for f in fronts]).reshape(m, 3)
    return {"n_nodes": n, "n_ghost": m, "node_pos": pos, "node_step": np.arange(1, n + 1), "adj": adj, "ghost_pos": gpos,
            "ghost_fronts": fronts, "cur_node": int(rng.integers(n)) if cur is None else cur, "cur_pos": np.zeros(3), "cur_heading": 0.0}


def random_logits(n, m, G, rng):
    """fp32 row: [stop] and the ghosts N(0, 2), visited nodes -inf with probability 1/2, the padding -inf"""
    l = np.full(G, -INF, dtype=np.float32)
    l[:1 + n + m] = (2.0 * rng.standard_normal(1 + n + m)).astype(np.float32)
    l[1:1 + n][rng.random(n) < 0.5] = -INF
    return l


def midpoint_uniform(logits, rng):
    """u0 (fp32): the midpoint of the cdf interval of a random entry with probability >= 1e-3"""
    p = softmax64(logits)
    cdf = np.concatenate(([0.0], np.cumsum(p)))
    k = int(rng.choice(np.nonzero(p >= 1e-3)[0]))
    return np.float32(0.5 * (cdf[k] + cdf[k + 1]) / cdf[-1])


def make_case(ns, ms, G=None, seed=0, sample=True, sample_ratio=0.25, force_stop=False, S=None, name=""):
    """A batch of len(ns) random episodes (redrawn until check_conditions passes; none is left out) -> dict with the packed batch,
    logits [B,G] fp32, table [S,64] fp32 (random scores in the rows' first n entries, -inf elsewhere), slots (a permutation prefix),
    uniforms [B,2] / teacher [B] (sample) and the per-episode reference results."""
    rng = np.random.default_rng(seed)
    B = len(ns)
    need = max(1 + n + m for n, m in zip(ns, ms))
    G = need if G is None else G
    S = B if S is None else S
    slots = rng.permutation(S)[:B].astype(np.int32)
    table = np.full((S, 64), -INF, dtype=np.float32)
    eps, logits, uni, teacher, refs = [], np.zeros((B, G), np.float32), np.zeros((B, 2), np.float32), np.zeros(B, np.int64), []
    for b, (n, m) in enumerate(zip(ns, ms)):
        for attempt in range(200):
            ep = random_episode(n, m, rng)
            l = random_logits(n, m, G, rng)
            row = np.full(64, -INF, dtype=np.float32)
            row[:n] = rng.uniform(0.0, 0.9, n).astype(np.float32)
            u = (midpoint_uniform(l, rng), np.float32(rng.random())) if sample else None
            t = int(rng.choice([0] + list(range(1 + n, 1 + n + m)))) if m else IGNORE
            try:
                r = check_conditions(ep, l, row, u, t if sample else None, sample_ratio, force_stop, name=f"{name}[{b}]")
            except AssertionError:
                continue
            if r["flags"] & ~STOP:
                continue
            break
        else:
            raise AssertionError(f"{name}[{b}]: no draw met the conditions")
        eps.append(ep); refs.append(r)
        logits[b], table[slots[b]], teacher[b] = l, row, t
        if sample:
            uni[b] = u
    return dict(eps=eps, batch=pack_batch(eps), logits=logits, table=table, slots=slots, uniforms=uni if sample else None,
                teacher=teacher if sample else None, sample_ratio=sample_ratio, force_stop=force_stop, refs=refs, G=G, S=S)


# ---- rollouts: one driver for the real GraphMap + the reference's statements, GraphMapLite + this restatement, and the device ------------
CFG = dict(max_len=6, sample_ratio=0.25, consume_ghost=True, back_algo="control", tryout=True, loc_noise=0.5, merge_ghost=True)


def drive(make_gmap, plan, decide_step, num_envs, cfg=CFG):
    """The rollout loop around the decision (ss_trainer_ETP.py:842-871, 1036-1044, reduced to what the decision depends on): per step
    update every active graph at the plan's pose and candidates, ask the plan for logits / teacher / uniforms, decide, move every
    agent that goes on to its ghost, pause the ones that stopped.  decide_step(gmaps, cur_vp, prev_vp, active, logits, teacher,
    uniforms, feedback, stepk) -> (cpu_a_t, env_actions) applies the loop's side effects.  -> the log (a list of JSON-able steps)."""
    gmaps = [make_gmap() for _ in range(num_envs)]
    prev_vp, active = [None] * num_envs, list(range(num_envs))
    cur_pos = {s: np.asarray(plan.start(s), dtype=np.float64) for s in active}
    log = []
    for stepk in range(cfg["max_len"]):
        feedback = plan.feedback(stepk)
        cur_vp, cands = [], []
        for i, s in enumerate(active):
            c = np.asarray(plan.cands(s, stepk, cur_pos[s]), dtype=np.float64).reshape(-1, 3)
            vp = str(len(gmaps[i].node_pos))
            gmaps[i].update_graph(prev_vp[i], stepk + 1, vp, cur_pos[s].copy(), 0.0, [f"{vp}_{j}" for j in range(len(c))],
                                  [x for x in c], [0.0] * len(c), [None] * len(c))
            cur_vp.append(vp); cands.append(c.tolist())
        vp_ids = [[None] + list(g.node_pos.keys()) + list(g.ghost_pos.keys()) for g in gmaps]
        B, G = len(active), max(len(v) for v in vp_ids)
        logits, teacher, uni = np.full((B, G), -INF, dtype=np.float32), np.zeros(B, np.int64), np.zeros((B, 2), np.float32)
        for i, s in enumerate(active):
            l, teacher[i], uni[i] = plan.policy(s, stepk, gmaps[i], cur_vp[i])
            logits[i, :len(l)] = l
        entry = dict(stepk=stepk, feedback=feedback, slots=list(active), cur_vp=list(cur_vp), cur_pos=[cur_pos[s].tolist() for s in active],
                     cands=cands, logits=logits.astype(np.float64).tolist(), teacher=teacher.tolist(),
                     uniforms=uni.astype(np.float64).tolist())
        a_t, env_actions = decide_step(gmaps, cur_vp, prev_vp, active, logits, teacher, uni, feedback, stepk)
        acts = []
        for ea in env_actions:
            a = dict(ea["action"])
            for k in ("stop_pos", "front_pos", "ghost_pos"):
                if k in a:
                    a[k] = np.asarray(a[k], dtype=np.float64).tolist()
            if a["back_path"] is not None:
                a["back_path"] = [[vp, np.asarray(pos, dtype=np.float64).tolist()] for vp, pos in a["back_path"]]
            v = ea["vis_info"]
            a["vis"] = None if v is None else [len(v["nodes"]), len(v["ghosts"]), np.asarray(v["predict_ghost"], dtype=np.float64).tolist()]
            acts.append(a)
        entry.update(a_t=[int(x) for x in a_t], actions=acts, prev_vp=list(prev_vp),
                     ghosts_after=[list(g.ghost_pos.keys()) for g in gmaps],
                     stop_scores=[[[vp, float(sc)] for vp, sc in g.node_stop_scores.items()] for g in gmaps])
        log.append(entry)
        for i in reversed(range(len(active))):
            if acts[i]["act"] == 0:
                active.pop(i); gmaps.pop(i); prev_vp.pop(i)
                if hasattr(decide_step, "pause"):
                    decide_step.pause(i)
            else:
                cur_pos[active[i]] = np.asarray(acts[i]["ghost_pos"], dtype=np.float64)
        if not active:
            break
    return log


class RefStep:
    """decide_step of `drive` from episode_ref: the restated loop :908-977 with its side effects; `mut` plants one of MUTATIONS"""

    def __init__(self, num_envs, cfg=CFG, mut=None):
        self.table = np.full((num_envs, 64), -INF)
        self.cfg, self.mut = cfg, mut

    def __call__(self, gmaps, cur_vp, prev_vp, active, logits, teacher, uni, feedback, stepk):
        cfg, mut = self.cfg, self.mut
        a_t, env_actions = [], []
        for i, gmap in enumerate(gmaps):
            ep = pack_episode(gmap, cur_vp[i], np.zeros(3), 0.0)
            slot = i if mut == "wrong_slot" else active[i]
            sample = feedback == "sample"
            r = episode_ref(ep, logits[i], self.table[slot], uni[i] if sample else None, int(teacher[i]) if sample else None,
                            cfg["sample_ratio"], stepk == cfg["max_len"] - 1, mut)
            assert not r["flags"] & ~STOP, r["flags"]
            self.table[slot] = r["row"]
            gmap.node_stop_scores[cur_vp[i]] = r["stop_prob"]
            nodes, ghosts = list(gmap.node_pos.keys()), list(gmap.ghost_pos.keys())
            back = [(nodes[k], gmap.node_pos[nodes[k]]) for k in r["path"]] if cfg["back_algo"] == "control" else None
            a_t.append(r["action"])
            if r["flags"] & STOP:
                svp = nodes[r["stop_node"]]
                env_actions.append({"action": {"act": 0, "cur_vp": cur_vp[i], "stop_vp": svp, "stop_pos": gmap.node_pos[svp],
                                               "back_path": back, "tryout": cfg["tryout"]},
                                    "vis_info": {"nodes": list(gmap.node_pos.values()), "ghosts": list(gmap.ghost_aug_pos.values()),
                                                 "predict_ghost": gmap.node_pos[svp]}})
            else:
                gvp, fvp = ghosts[r["ghost"]], nodes[r["target"]]
                env_actions.append({"action": {"act": 4, "cur_vp": cur_vp[i], "front_vp": fvp, "front_pos": gmap.node_pos[fvp],
                                               "ghost_vp": gvp, "ghost_pos": gmap.ghost_aug_pos[gvp], "back_path": back,
                                               "tryout": cfg["tryout"]}, "vis_info": None})
                prev_vp[i] = fvp
                if cfg["consume_ghost"] and mut != "keep_ghost":
                    gmap.delete_ghost(gvp)
        return np.asarray(a_t, dtype=np.int64), env_actions


class ReplayPlan:
    """the plan of a recorded log: poses, candidates, logits, teacher labels and uniforms as stored"""

    def __init__(self, log):
        self.log = log
        self.at = {(e["stepk"], s): (e, i) for e in log for i, s in enumerate(e["slots"])}

    def start(self, s):
        e, i = self.at[(0, s)]
        return e["cur_pos"][i]

    def feedback(self, stepk):
        return self.log[stepk]["feedback"]

    def cands(self, s, stepk, cur_pos):
        e, i = self.at[(stepk, s)]
        assert np.allclose(cur_pos, e["cur_pos"][i], rtol=0, atol=1e-6), (stepk, s, cur_pos, e["cur_pos"][i])
        return e["cands"][i]

    def policy(self, s, stepk, gmap, cur_vp):
        e, i = self.at[(stepk, s)]
        L = 1 + len(gmap.node_pos) + len(gmap.ghost_pos)
        return (np.asarray(e["logits"][i][:L], dtype=np.float32), int(e["teacher"][i]), np.asarray(e["uniforms"][i], dtype=np.float32))


class RandomPlan:
    """random rollouts: 1 .. 4 candidates per step at 1.5 .. 3 from the agent (one of them now and then on an earlier node, which
    becomes an edge), N(0, 2) logits on [stop] and the ghosts, -inf on the visited nodes, a random ghost or 0 as the teacher label,
    u0 at the midpoint of a cdf cell; steps >= argmax_from run feedback 'argmax'"""

    def __init__(self, seed, argmax_from=4, stop_bias=-1.0):
        self.rng = np.random.default_rng(seed)
        self.argmax_from, self.stop_bias = argmax_from, stop_bias
        self.visited = {}

    def start(self, s):
        return [10.0 * s, 0.0, 0.0]

    def feedback(self, stepk):
        return "sample" if stepk < self.argmax_from else "argmax"

    def cands(self, s, stepk, cur_pos):
        rng = self.rng
        seen = self.visited.setdefault(s, [])
        out = []
        for _ in range(int(rng.integers(1, 5))):
            a, d = rng.uniform(0, 2 * np.pi), rng.uniform(1.5, 3.0)
            out.append(cur_pos + [d * np.sin(a), 0.0, d * np.cos(a)])
        if len(seen) >= 2 and rng.random() < 0.5:
            out.append(seen[int(rng.integers(len(seen) - 1))] + rng.uniform(-0.1, 0.1, 3) * [1, 0, 1])
        seen.append(np.array(cur_pos, dtype=np.float64))
        return out

    def policy(self, s, stepk, gmap, cur_vp):
        rng = self.rng
        n, m = len(gmap.node_pos), len(gmap.ghost_pos)
        l = np.full(1 + n + m, -INF, dtype=np.float32)
        l[0] = np.float32(2.0 * rng.standard_normal() + self.stop_bias)
        l[1 + n:] = (2.0 * rng.standard_normal(m)).astype(np.float32)
        teacher = int(rng.choice([0] + list(range(1 + n, 1 + n + m)) * 3)) if m else IGNORE
        return l, teacher, np.array([midpoint_uniform(l, rng), rng.random()], dtype=np.float32)


def compare_logs(got, want, name="", pos_tol=1e-6, prob_tol=1e-6):
    """the decisions of two logs: cpu_a_t, the env_actions (names equal, positions at pos_tol, back_path names equal), vis_info,
    prev_vp, the ghosts left and the stop scores, at every step"""
    assert len(got) == len(want), f"{name}: {len(got)} steps against {len(want)}"
    for g, w in zip(got, want):
        at = f"{name} step {w['stepk']}"
        assert g["slots"] == w["slots"] and g["cur_vp"] == w["cur_vp"], at
        assert g["a_t"] == w["a_t"], f"{at}: cpu_a_t {g['a_t']} against {w['a_t']}"
        for i, (ga, wa) in enumerate(zip(g["actions"], w["actions"])):
            assert sorted(ga.keys()) == sorted(wa.keys()), f"{at}[{i}]: keys {sorted(ga.keys())} against {sorted(wa.keys())}"
            for k, wv in wa.items():
                gv = ga[k]
                if k in ("stop_pos", "front_pos", "ghost_pos"):
                    assert np.allclose(gv, wv, rtol=0, atol=pos_tol), f"{at}[{i}]: {k} {gv} against {wv}"
                elif k == "back_path":
                    assert (gv is None) == (wv is None), f"{at}[{i}]: back_path {gv} against {wv}"
                    if wv is not None:
                        assert [x[0] for x in gv] == [x[0] for x in wv], f"{at}[{i}]: back_path {[x[0] for x in gv]} against {[x[0] for x in wv]}"
                        assert all(np.allclose(a[1], b[1], rtol=0, atol=pos_tol) for a, b in zip(gv, wv)), f"{at}[{i}]: back_path positions"
                elif k == "vis":
                    assert (gv is None) == (wv is None) and (wv is None or (gv[:2] == wv[:2] and np.allclose(gv[2], wv[2], rtol=0, atol=pos_tol))), \
                        f"{at}[{i}]: vis_info {gv} against {wv}"
                else:
                    assert gv == wv and type(gv) is type(wv), f"{at}[{i}]: {k} {gv!r} against {wv!r}"
        assert g["prev_vp"] == w["prev_vp"], f"{at}: prev_vp {g['prev_vp']} against {w['prev_vp']}"
        assert g["ghosts_after"] == w["ghosts_after"], f"{at}: ghosts left {g['ghosts_after']} against {w['ghosts_after']}"
        for gs, ws in zip(g["stop_scores"], w["stop_scores"]):
            assert [x[0] for x in gs] == [x[0] for x in ws], f"{at}: stop-score keys"
            assert np.allclose([x[1] for x in gs], [x[1] for x in ws], rtol=0, atol=prob_tol), f"{at}: stop scores {gs} against {ws}"


def load_fixture(path):
    z = np.load(path)
    return json.loads(str(z["log"])), json.loads(str(z["cfg"]))
