"""The embedding store on the MI355X: etp_pano_store_fwd / etp_pano_store_bwd (csrc/pano_store.hip) and graph_inputs.EmbedStore against
the fp64 restatement tests/pano_store_ref.py (pinned by tests/test_pano_store_ref_cpu.py), with its shape lists and its derived bounds
(no multiplier): candidate rows bit for bit, the mean inside gam(n) * sum |x| / n, the backward inside u |t| + u |t + c|.

Every output is pre-filled with a NaN bit pattern and carries guard rows; what a call must not touch comes back with those bits.
Each case is a handful of launches on a few rows.  The worst observed error / bound ratios go to profiles/pano_store_op_bounds.txt.

Worst ratios of the final library on an MI355X (profiles/pano_store_op_bounds.txt): mean rows 0.67, backward 0.996 (0.995 with
accumulate), the recorded rollout's gmap_img_fts 0.45 and d pano_embeds 0.42 on both routes, 0.43 behind the real forward_panorama."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib, graph_inputs  # noqa: E402
from etpnav_amd._lib import ptr  # noqa: E402
from etpnav_amd.graph_inputs import DeviceGraphMaps, EmbedStore, GraphMapLite  # noqa: E402
from tests import pano_store_ref as pr  # noqa: E402

DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "pano_store_small.npz")
PROFILE = os.path.join(os.path.dirname(HERE), "profiles", "pano_store_op_bounds.txt")
SENT = np.int32(0x7FC0BEEF)                                    # a NaN with a payload: arithmetic on it would change the bits
GUARD = 2                                                      # rows behind R / one episode behind B that no call may touch
WORST = {}


def stream():
    return torch.cuda.current_stream().cuda_stream


def sent(*shape):
    return torch.full(shape, int(SENT), dtype=torch.int32, device=DEV).view(torch.float32)


def bits(t):
    return t.view(torch.int32).cpu().numpy()


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def note(key, err, bound):
    nz = bound > 0
    WORST[key] = max(WORST.get(key, 0.0), float((err[nz] / bound[nz]).max()) if nz.any() else 0.0)


@pytest.fixture(scope="module", autouse=True)
def write_profile():
    yield
    if not WORST:
        return
    text = ("worst |device - fp64| / derived bound per check of tests/test_pano_store_gpu.py (a ratio <= 1 passes; candidate rows, zeros "
            "and untouched rows are compared bit for bit and do not appear)\n" + "".join(f"{k:42s} {WORST[k]:.4f}\n" for k in sorted(WORST)))
    try:                                                      # the kernels are deterministic: a rerun writes the same file
        with open(os.environ.get("ETP_PANO_STORE_BOUNDS_OUT", PROFILE), "w") as f:
            f.write(text)
    except OSError as e:                                      # a read-only checkout: the figures go to the log instead
        print(f"{PROFILE}: {e}\n{text}")


def run_fwd(c, R=None):
    R = c["R"] if R is None else R
    B, V, H = c["x"].shape
    t = [up(c[k]) for k in ("x", "masks", "types", "base", "ncand")]
    store, status = sent(R + GUARD, H), torch.full((B + 1,), -777, dtype=torch.int32, device=DEV)
    rc = _lib.lib().etp_pano_store_fwd(*[ptr(x) for x in t], B, V, H, ptr(store), R, ptr(status), stream())
    assert rc == 0, _lib.lib().etp_last_error()
    st = status.cpu().numpy()
    assert st[B] == -777
    return store, st[:B]


def check_fwd(c, key, R=None):
    """device store against the restatement run on a NaN store: NaN there = the sentinel's bits here; candidate rows bit-equal"""
    R = c["R"] if R is None else R
    B, V, H = c["x"].shape
    a = (c["x"], c["masks"], c["types"], c["base"], c["ncand"])
    want, st = pr.fwd(*a, np.full((R, H), np.nan))
    bound = pr.fwd_bound(*a, R)
    store, got_st = run_fwd(c, R)
    assert np.array_equal(got_st, st), (got_st, st)
    got_bits, got = bits(store), store.cpu().numpy().astype(np.float64)
    untouched = np.isnan(want)
    assert (got_bits[R:] == SENT).all(), "guard rows behind the store overwritten"
    assert (got_bits[:R][untouched] == SENT).all(), "a row the call must not touch was written"
    exact = ~untouched & (np.broadcast_to(bound.sum(1, keepdims=True), bound.shape) == 0)
    assert np.array_equal(got[:R][exact].astype(np.float32).view(np.int32), want[exact].astype(np.float32).view(np.int32)), "candidate rows are bit copies"
    mean = ~untouched & ~exact
    err = np.abs(got[:R] - want)
    assert (err[mean] <= bound[mean]).all(), f"mean rows: worst ratio {(err[mean] / bound[mean]).max():.3f}"
    note(key, err[mean], bound[mean])
    again, _ = run_fwd(c, R)
    assert np.array_equal(bits(again), got_bits), "a second run differs"
    return got_st


def run_bwd(c, accumulate, old=None, R=None):
    R = c["R"] if R is None else R
    B, V = c["masks"].shape
    H = c["d_store"].shape[1]
    t = [up(c[k]) for k in ("masks", "types", "base", "ncand")]
    ds = up(c["d_store"][:R])
    dx = sent(B + 1, V, H)
    if old is not None:
        dx[:B] = up(old)
    rc = _lib.lib().etp_pano_store_bwd(ptr(ds), *[ptr(x) for x in t], B, V, H, R, ptr(dx), accumulate, stream())
    assert rc == 0, _lib.lib().etp_last_error()
    assert (bits(dx[B:]) == SENT).all(), "guard episode behind d_pano_embeds overwritten"
    return dx[:B]


def check_bwd(c, key, R=None):
    R = c["R"] if R is None else R
    B, V = c["masks"].shape
    b = (c["masks"], c["types"], c["base"], c["ncand"])
    d_store = c["d_store"][:R]
    # accumulate == 0: everything is written; padded views and malformed episodes are +0.0, a lone candidate term is a bit copy
    want, bound = pr.bwd(d_store, *b, V), pr.bwd_bound(d_store, *b, V)
    dx = run_bwd(c, 0, R=R)
    got_bits, got = bits(dx), dx.cpu().numpy().astype(np.float64)
    exact = bound == 0
    assert np.array_equal(got_bits[exact], want[exact].astype(np.float32).view(np.int32)), "exact elements (zeros, copies) differ"
    err = np.abs(got - want)
    assert (err <= bound).all(), f"backward: worst ratio {(err[~exact] / bound[~exact]).max():.3f}"
    note(key + " bwd", err, bound)
    assert np.array_equal(bits(run_bwd(c, 0, R=R)), got_bits), "a second run differs"
    # accumulate == 1: added to what is there; malformed episodes keep their bits
    old = np.random.default_rng(3).standard_normal(want.shape).astype(np.float32)
    want, bound = pr.bwd(d_store, *b, V, d_pano=old, accumulate=1), pr.bwd_bound(d_store, *b, V, d_pano=old, accumulate=1)
    dx = run_bwd(c, 1, old=old, R=R)
    got = dx.cpu().numpy()
    bad = pr.flags(*b, R) != 0
    assert np.array_equal(got[bad].view(np.int32), old[bad].view(np.int32)), "accumulate: a malformed episode was touched"
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), f"backward, accumulate: worst ratio {(err[bound > 0] / bound[bound > 0]).max():.3f}"
    note(key + " bwd accumulate", err, bound)


# ---- the operators -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B,V", pr.CASES)
def test_operators_against_fp64(H, B, V):
    c = pr.make_case(H, B, V)
    assert not check_fwd(c, f"H{H} mean").any()
    check_bwd(c, f"H{H}")


@pytest.mark.parametrize("name", list(pr.malformed_cases()))
def test_malformed_episode_is_flagged_and_writes_nothing(name):
    c, flag = pr.malformed_cases()[name]
    assert check_fwd(c, "malformed mean").tolist() == [0, flag, 0]
    check_bwd(c, "malformed")


def test_store_exactly_fitting_and_one_row_short():
    c = pr.make_case(256, 3, 5)
    top = int((c["base"] + 1 + c["ncand"]).max())
    last = int(np.argmax(c["base"] + 1 + c["ncand"]))
    assert not check_fwd(c, "fitting mean", R=top).any()
    check_bwd(c, "fitting", R=top)
    st = check_fwd(c, "fitting mean", R=top - 1)
    assert st[last] == pr.ERR_ROW and st.sum() == pr.ERR_ROW
    check_bwd(c, "fitting", R=top - 1)


def test_host_refusals_leave_every_buffer_as_it_was():
    c = pr.make_case(256, 3, 5)
    B, V, H, R = 3, 5, 256, c["R"]
    t = {k: up(c[k]) for k in ("x", "masks", "types", "base", "ncand")}
    store, status, dx, ds = sent(R + GUARD, H), torch.full((B,), -777, dtype=torch.int32, device=DEV), sent(B, V, H), up(c["d_store"])
    L = _lib.lib()

    def fwd(**kw):
        a = dict(x=ptr(t["x"]), masks=ptr(t["masks"]), types=ptr(t["types"]), base=ptr(t["base"]), ncand=ptr(t["ncand"]), B=B, V=V, H=H,
                 store=ptr(store), R=R, status=ptr(status))
        a.update(kw)
        return L.etp_pano_store_fwd(a["x"], a["masks"], a["types"], a["base"], a["ncand"], a["B"], a["V"], a["H"], a["store"], a["R"], a["status"], stream())

    def bwd(**kw):
        a = dict(ds=ptr(ds), masks=ptr(t["masks"]), types=ptr(t["types"]), base=ptr(t["base"]), ncand=ptr(t["ncand"]), B=B, V=V, H=H, R=R,
                 dx=ptr(dx), acc=0)
        a.update(kw)
        return L.etp_pano_store_bwd(a["ds"], a["masks"], a["types"], a["base"], a["ncand"], a["B"], a["V"], a["H"], a["R"], a["dx"], a["acc"], stream())

    for kw in (dict(H=128), dict(H=1024), dict(V=0), dict(V=65), dict(B=0), dict(R=0), dict(x=ptr(t["x"]) + 4), dict(store=ptr(store) + 8),
               dict(x=None), dict(masks=None), dict(types=None), dict(base=None), dict(ncand=None), dict(store=None), dict(status=None)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(H=128), dict(V=0), dict(V=65), dict(B=0), dict(R=0), dict(ds=ptr(ds) + 4), dict(dx=ptr(dx) + 8), dict(acc=2), dict(ds=None),
               dict(dx=None), dict(masks=None)):
        assert bwd(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (bits(store) == SENT).all() and (bits(dx) == SENT).all() and (status.cpu().numpy() == -777).all()


# ---- the store route: the recording of the real GraphMap -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    z = np.load(FIXTURE)
    d = {k: z[k] for k in z.files}
    d["plan"], d["names"] = json.loads(str(d["plan"])), json.loads(str(d["names"]))
    T, B, V, H = d["pano"].shape
    d["G"], d["loc_noise"] = int(d["G"]), float(d["loc_noise"])
    d["W"] = pr.fixture_w(int(d["w_seed"]), T, B, d["G"], H)
    d["entries"], d["alloc"], d["R"] = pr.replay_plan(d["plan"], lambda: GraphMapLite(False, d["loc_noise"], True, 0), snap=pr.entry_rows)
    a = (d["pano"], d["masks"], d["types"], d["entries"], d["alloc"], d["R"], d["W"])
    d["fwd_bound"], d["bwd_bound"] = pr.route_fwd_bound(*a), pr.route_bwd_bound(*a)
    d["detached"] = pr.route(*a, mut="detach_steps")[1]
    return d


def replay_on_device(fx, route, xs):
    """the fixture's rollout through EmbedStore and either DeviceGraphMaps ("device") or GraphMapLite in device-store mode + gather_rows
    ("lite") -> (gmap_img_fts of every step, the store)"""
    T, B, V, H = fx["pano"].shape
    store = EmbedStore(fx["R"] + 3, H, DEV)
    maps = DeviceGraphMaps(B, DEV, False, fx["loc_noise"], True, 0.0) if route == "device" else None
    lites = [GraphMapLite(False, fx["loc_noise"], True, 0) for _ in range(B)]
    gm = maps.gmaps if maps is not None else lites
    fts, heading = [], [0.0] * B
    for t, step in enumerate(fx["plan"]):
        ks = [len(c) for c in step["cand_pos"]]
        cur_rows, cand_rows = store.append(xs[t], up(fx["masks"][t]), up(fx["types"][t]), ks)
        assert cur_rows == fx["alloc"][t][0].tolist() and [len(r) for r in cand_rows] == ks
        for b in range(B):
            if step["delete"][b] is not None:
                gm[b].delete_ghost(step["delete"][b])
        cur_vp = [str(len(g.node_pos)) for g in gm]
        cand_pos = [[np.asarray(p, dtype=np.float64) for p in c] for c in step["cand_pos"]]
        if maps is not None:
            maps.update(step["prev_vp"], t + 1, cur_vp, np.asarray(step["cur_pos"], dtype=np.float64), heading, cand_pos, cur_rows, cand_rows)
            f = maps.img_fts(store, fx["G"])
        else:
            for b, g in enumerate(lites):
                g.update_graph(step["prev_vp"][b], t + 1, cur_vp[b], np.asarray(step["cur_pos"][b], dtype=np.float64), cur_rows[b],
                               [f"{cur_vp[b]}_{k}" for k in range(ks[b])], cand_pos[b], cand_rows[b], [None] * ks[b])
            f = graph_inputs.gather_rows(store, lites, [0] * B, fx["G"])
        assert [pr.entry_names(g) for g in gm] == fx["names"][t]
        fts.append(f)
    return fts, store


@pytest.mark.parametrize("route", ["device", "lite"])
def test_fixture_rollout_forward_and_backward_through_the_store(fx, route):
    T, B, V, H = fx["pano"].shape
    xs = [up(fx["pano"][t].astype(np.float32)).requires_grad_(True) for t in range(T)]
    fts, store = replay_on_device(fx, route, xs)
    loss = sum((f * up(fx["W"][t].astype(np.float32))).sum() for t, f in enumerate(fts))
    loss.backward()
    store.check()
    assert store.rows_used == fx["R"] and not store.buf[fx["R"]:].any()
    for t in range(T):
        got = fts[t].detach().cpu().numpy().astype(np.float64)
        for b in range(B):
            n = fx["n_entries"][t, b]
            err, bound = np.abs(got[b, :n] - fx["fts"][t, b, :n]), fx["fwd_bound"][t][b, :n]
            assert (err <= bound).all(), (t, b, float((err / np.maximum(bound, 1e-300)).max()))
            note(f"fixture {route} gmap_img_fts", err, bound)
            assert not got[b, n:].any()
        d = xs[t].grad.cpu().numpy().astype(np.float64)
        err, bound = np.abs(d - fx["d_pano"][t]), fx["bwd_bound"][t]
        assert (err <= bound).all(), (t, float((err[bound > 0] / bound[bound > 0]).max()))
        note(f"fixture {route} d pano_embeds", err, bound)
    # step 0's gradient holds what steps 1 and 2 sent back: without it the result is far outside the bound
    d0 = xs[0].grad.cpu().numpy().astype(np.float64)
    assert (np.abs(d0 - fx["detached"][0]) > fx["bwd_bound"][0] + 1e-3).any()


def test_no_grad_builds_no_graph_and_check_names_call_and_episode(fx):
    T, B, V, H = fx["pano"].shape
    xs = [up(fx["pano"][t].astype(np.float32)).requires_grad_(True) for t in range(T)]
    with torch.no_grad():
        fts, store = replay_on_device(fx, "device", xs)
    assert all(f.grad_fn is None and not f.requires_grad for f in fts) and all(b.grad_fn is None for b in store._blocks)
    assert not store.rows().requires_grad
    fts2, _ = replay_on_device(fx, "device", [x.detach() for x in xs])          # inputs without a gradient: nothing to build either
    assert all(not f.requires_grad for f in fts2)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(fts, fts2))
    # a count that does not match nav_types is flagged on the device and raised by check(), naming call and episode
    s = EmbedStore(16, H, DEV)
    s.append(xs[0].detach(), up(fx["masks"][0]), up(fx["types"][0]), [len(c) for c in fx["plan"][0]["cand_pos"]])
    ks = [len(c) for c in fx["plan"][1]["cand_pos"]]
    ks[0] -= 1
    cur_rows, _ = s.append(xs[1].detach(), up(fx["masks"][1]), up(fx["types"][1]), ks)
    with pytest.raises(_lib.EtpError, match="call 1 episode 0: flags 4"):
        s.check()
    assert not s.buf[cur_rows[0]:cur_rows[0] + 1 + ks[0]].any() and s.buf[cur_rows[1]].any()
    s.check()                                                 # already reported
    s.reset()
    assert s.rows_used == 0 and not s.buf.any()


def test_forward_panorama_in_front_reaches_the_encoder_as_the_eager_store_does():
    """The real forward_panorama at B = 2, two steps, loss sum_t (gmap_img_fts_t * W_t).sum(): the store built by EmbedStore against the
    store built by the trainer's torch statements (mean, boolean selection, torch.cat) feeding the same gather.
    d pano_embeds of the EmbedStore route (what _PanoFn.backward receives) is held to the fp64 route within route_bwd_bound.  The
    encoder's backward is one linear map applied to two inputs that agree to about 1e-7 relative; the repository holds this fp32 chain
    to 2e-3 relative against the oracle (tests/test_planner_gpu.py), so the two routes' parameter gradients are asked to agree to 1e-5
    relative L2: a hundred times tighter than that tolerance, a hundred times looser than the perturbation."""
    from oracle import planner_oracle as po
    from etpnav_amd.planner import GlocalTextPathNavCMT
    cfg = po.PlannerConfig.r2r(vocab_size=2048, num_l_layers=1, num_pano_layers=1, num_x_layers=1)
    model = GlocalTextPathNavCMT(cfg.to_dict(), dtype=torch.float32, device=DEV)
    model.load_state_dict(po.init_params(cfg, seed=2), strict=True)
    model.eval()
    T, B, V, H = 2, 2, 7, 768
    batches = [{k: v.to(DEV) for k, v in po.make_batch(cfg, B=B, L=8, V=V, G=6, seed=40 + t, ragged=True).items()} for t in range(T)]
    types_h = [bt["nav_types"].cpu().numpy() for bt in batches]
    results = {}
    for route in ("store", "eager"):
        model.zero_grad()
        lites = [GraphMapLite(False, 0.5, True, 0) for _ in range(B)]
        store, eager, hooks, loss, used = EmbedStore(64, H, DEV), None, {}, 0.0, 0
        panos, masks, entries, alloc, W = [], [], [], [], []
        for t, bt in enumerate(batches):
            pano, pmask = model.forward_panorama(bt["rgb_fts"], bt["dep_fts"], bt["loc_fts"], bt["nav_types"], bt["view_lens"])
            pano.register_hook(lambda g, t=t: hooks.__setitem__(t, g.detach().cpu().numpy().astype(np.float64)))
            ks = [int((types_h[t][b] == 1).sum()) for b in range(B)]
            base, cand_rows, used = pr.allocate(used, ks)
            if route == "store":
                cur_rows, cr = store.append(pano, pmask, bt["nav_types"], ks)
                assert cur_rows == base.tolist() and cr == cand_rows
            else:
                m = pmask.to(pano.dtype)
                avg = (pano * m[..., None]).sum(1) / m.sum(1, keepdim=True)
                rows = [r for b in range(B) for r in (avg[b:b + 1], pano[b][bt["nav_types"][b] == 1])]
                eager = torch.cat(([eager] if eager is not None else []) + rows, 0)
            for b, g in enumerate(lites):
                vp = str(len(g.node_pos))
                pos = [np.array([3.0 * t + 1.0 + k, 0.0, 10.0 * b + 2.0 * k]) for k in range(ks[b])]       # far apart: every candidate a ghost
                g.update_graph(None if t == 0 else str(t - 1), t + 1, vp, np.array([3.0 * t, 0.0, 10.0 * b]), int(base[b]),
                               [f"{vp}_{k}" for k in range(ks[b])], pos, cand_rows[b], [None] * ks[b])
            G = 1 + max(len(pr.entry_names(g)) for g in lites)
            f = graph_inputs.gather_rows(store if route == "store" else eager, lites, [0] * B, G)
            W.append(np.random.default_rng(t).standard_normal((B, G, H)).astype(np.float32))
            loss = loss + (f * up(W[t])).sum()
            panos.append(pano.detach().cpu().numpy().astype(np.float64)); masks.append(pmask.cpu().numpy())
            entries.append([pr.entry_rows(g) for g in lites]); alloc.append((base, np.asarray(ks, dtype=np.int32)))
        loss.backward()
        torch.cuda.synchronize()
        store.check()
        grads = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}
        results[route] = (hooks, grads, (np.stack(panos), np.stack(masks), np.stack(types_h), entries, alloc, used, [w.astype(np.float64) for w in W]))
    a = results["store"][2]
    exact, bound = pr.route(*a)[1], pr.route_bwd_bound(*a)
    for t in range(T):
        err = np.abs(results["store"][0][t] - exact[t])
        assert (err <= bound[t]).all(), (t, float((err[bound[t] > 0] / bound[t][bound[t] > 0]).max()))
        note("forward_panorama d pano_embeds", err, bound[t])
    ga, ge = results["store"][1], results["eager"][1]
    live = [k for k in ge if ge[k].norm() > 0]
    assert len(live) >= 4, live
    for k in live:
        assert (ga[k] - ge[k]).norm() <= 1e-5 * ge[k].norm(), (k, float((ga[k] - ge[k]).norm() / ge[k].norm()))
