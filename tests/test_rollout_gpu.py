"""The fine-tuning rollout loss (csrc/rollout_loss.hip), RolloutLoss and RolloutDriver (etpnav_amd/rollout.py) on the device, against the
float64 restatement and the derived bounds of tests/rollout_ref.py (no multiplier; the module docstring there has the derivations).

Operator level: every (B, G) of rollout_ref.cases() with T in {1, 3, 15} steps and a shrinking B, logits at 0 / +-80 with -inf columns,
none / some / all rows ignored, labels at column 0 and G - 1; one stacked call of 15 * 33 rows.  Outputs start as payload NaN inside
guarded buffers, inputs must come back unchanged, counts are exact and a second run is bit-identical.
RolloutLoss: its gradients are the direct launches' bits, the recording of the reference trainer's statements is replayed, and no
device-to-host copy happens before record().
RolloutDriver: fp32, small native encoders, 3 scripted environments, max_len 4, fixed uniforms, both fuse_pano_inputs settings, against
rollout_ref.hand_composed_rollout (the loop a user composes from the public pieces, with torch's loss).

ETP_ROLLOUT_BOUNDS_OUT=<path> writes the worst ratios there (profiles/rollout_loss_op_bounds.txt is such a file).
"""
import os
import random
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from etpnav_amd import _lib, rollout
from tests import eval_ref as er
from tests import rollout_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENTINEL = 0x4D4D4D4D
NAN_BITS = 0x7FC12345
F64 = torch.float64


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    out = os.environ.get("ETP_ROLLOUT_BOUNDS_OUT")
    if out and rr.WORST:
        with open(out, "w") as f:
            f.write("worst err / bound per case and tensor (tests/test_rollout_gpu.py; bounds: tests/rollout_ref.py, no multiplier)\n")
            f.write(rr.worst_table() + "\n")


class Guarded:
    """n 4-byte words of payload NaN (or `init`) between GUARD sentinel words on either side"""

    def __init__(self, shape, dtype=torch.float32, init=None):
        n = int(np.prod(shape))
        words = n * (2 if dtype in (torch.int64, torch.float64) else 1)
        self.buf = torch.full((words + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.buf[GUARD:GUARD + words] = NAN_BITS
        self.t = self.buf[GUARD:GUARD + words].view(dtype).view(*shape)
        if init is not None:
            self.t.copy_(init)
        self.ref = self.buf.clone()

    def check(self, name):
        assert torch.equal(self.buf[:GUARD], self.ref[:GUARD]) and torch.equal(self.buf[-GUARD:], self.ref[-GUARD:]), f"{name}: a guard word changed"

    def intact(self, name):
        assert torch.equal(self.buf, self.ref), f"{name}: a refused call wrote"


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32 if t.element_size() == 4 else torch.int64)


def read_record(g):
    return rollout.unpack_record(g.t.cpu().numpy().tobytes())


def run_direct(steps, w, upstream=None, name=""):
    """the three entry points over a rollout, every output in a guarded buffer -> (loss [1], [dlogits], record dict, [row_nll])"""
    rec = Guarded((8,), torch.int64, init=torch.zeros(8, dtype=torch.int64))
    loss, log = Guarded((1,)), Guarded((3,), torch.int64, init=torch.zeros(3, dtype=torch.int64))
    nll = [Guarded((x.shape[0],)) for x, _ in steps]
    dl = [Guarded(tuple(x.shape)) for x, _ in steps]
    keep = [(x.clone(), y.clone()) for x, y in steps]
    for (x, y), g in zip(steps, nll):
        rollout.rollout_ce_fwd(x, y, rec.t, rr.IGNORE, g.t)
    rollout.rollout_loss(rec.t, w, loss.t, log.t)
    up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=DEV)
    for (x, y), g in zip(steps, dl):
        rollout.rollout_ce_bwd(x, y, rec.t, w, up, rr.IGNORE, g.t)
    torch.cuda.synchronize()
    for g in [rec, loss, log] + nll + dl:
        g.check(name)
    for (x, y), (x0, y0) in zip(steps, keep):
        assert torch.equal(bits(x), bits(x0)) and torch.equal(y, y0), f"{name}: an input changed"
    s, n, nf = struct.unpack(rollout.LOG_FMT, log.t.cpu().numpy().tobytes())
    assert (n, nf) == (1, 0) and s == float(loss.t.item()), f"{name}: the log holds {(s, n, nf)}, the loss {float(loss.t.item())}"
    return loss.t.clone(), [g.t.clone() for g in dl], read_record(rec), [g.t.clone() for g in nll]


CASES = rr.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_operators_against_the_restatement(case):
    name, B, G, T, shift, ign, w = case
    steps = rr.make_steps(B, G, T, shift, ign, CASES.index(case), DEV)
    host = [(x.cpu(), y.cpu()) for x, y in steps]
    loss, dls, rec, nll = run_direct(steps, w, name=name)
    for t, ((x, y), v) in enumerate(zip(host, nll)):
        q = er.tail(x, y, rr.IGNORE)
        assert bool((v.cpu()[~q["keep"]] == 0).all()), f"{name} step {t}: an ignored row's nll is not 0"
        rr.within((name, "row_nll"), v.cpu(), q["nll"], er.nll_bound(q, er.sap_depth(G)))
    rr.check_loss(name, loss, host, w)
    rr.check_dlogits(name, dls, host, w)
    rr.check_record(name, rec, host)
    rr.check_record(name + " (own rows)", rec, host, row_nll=nll)
    loss2, dls2, rec2, nll2 = run_direct(steps, w, name=name + " second run")
    assert torch.equal(bits(loss), bits(loss2)) and rec == rec2, f"{name}: a second run differs"
    for a, b in zip(dls + nll, dls2 + nll2):
        assert torch.equal(bits(a), bits(b)), f"{name}: a second run differs"


def test_one_stacked_call_takes_every_row_in_row_order():
    T, B, G = rr.STACKED
    steps = rr.make_steps(B, G, T, 80.0, "some", 5, DEV)
    st = rr.stacked(steps)
    assert st[0][0].shape[0] > 256
    host = [(x.cpu(), y.cpu()) for x, y in st]
    loss, dls, rec, nll = run_direct(st, 0.37, name="stacked")
    rr.check_loss("stacked", loss, host, 0.37)
    rr.check_dlogits("stacked", dls, host, 0.37)
    rr.check_record("stacked", rec, host, calls=1)
    assert rec["n_steps"] == 1 and rec["n_actions"] == sum(rr.shrinking(B, T))
    # the same rows step by step: the same row values, the same scale, hence the same gradient bits; the double sum in the same order
    loss_s, dls_s, rec_s, nll_s = run_direct(steps, 0.37, name="stepwise")
    assert torch.equal(bits(torch.cat(nll_s)), bits(nll[0])) and torch.equal(bits(torch.cat(dls_s)), bits(dls[0]))
    assert rec_s["n_steps"] == T and (rec_s["n_actions"], rec_s["n_counted"]) == (rec["n_actions"], rec["n_counted"])
    rr.check_record("stepwise (own rows)", rec_s, [(x.cpu(), y.cpu()) for x, y in steps], row_nll=nll_s)


@pytest.mark.parametrize("upstream", [0.5, 0.3])
def test_the_upstream_gradient_scales_on_the_device(upstream):
    steps = rr.make_steps(7, 65, 3, 0.0, "some", 9, DEV)
    _, dls, _, _ = run_direct(steps, -2.5, upstream=upstream, name=f"upstream {upstream}")
    rr.check_dlogits(f"upstream {upstream}", dls, [(x.cpu(), y.cpu()) for x, y in steps], -2.5, upstream=upstream)


def test_special_rows_and_the_empty_record():
    inf = float("inf")
    x = torch.tensor([[0.5, -inf, 1.0, 2.0], [1.0, 2.0, 3.0, -inf], [0.0, 0.0, 0.0, 0.0], [1.0, -1.0, 0.5, 0.25], [0.0, 1.0, 2.0, 3.0]],
                     dtype=torch.float32, device=DEV)
    y = torch.tensor([1, 2, 10 ** 12, -5, rr.IGNORE], dtype=torch.int64, device=DEV)          # on -inf; fine; far outside; negative; ignored
    rec, nll, dl, loss = Guarded((8,), torch.int64, init=torch.zeros(8, dtype=torch.int64)), Guarded((5,)), Guarded((5, 4)), Guarded((1,))
    rollout.rollout_ce_fwd(x, y, rec.t, rr.IGNORE, nll.t)
    rollout.rollout_ce_bwd(x, y, rec.t, 1.0, None, rr.IGNORE, dl.t)
    rollout.rollout_loss(rec.t, 1.0, loss.t)
    torch.cuda.synchronize()
    v, d, r = nll.t.cpu(), dl.t.cpu(), read_record(rec)
    assert v[0] == inf and torch.isfinite(v[1]) and torch.isnan(v[2]) and torch.isnan(v[3]) and v[4] == 0
    assert (r["n_actions"], r["n_counted"], r["n_steps"], r["n_nonfinite"]) == (5, 4, 1, 3) and np.isnan(r["loss_sum"])
    assert bool(torch.isnan(d[2]).all()) and bool(torch.isnan(d[3]).all()) and bool((d[4] == 0).all()) and d[1, 3] == 0
    assert bool(torch.isfinite(d[1]).all()) and bool(torch.isnan(loss.t.cpu()).all())
    for g in (rec, nll, dl, loss):
        g.check("special rows")
    # a record that no step has advanced: the loss is exactly 0, the scale of the backward is 0, the log takes the 0
    rec0, loss0, log0, dl0 = Guarded((8,), torch.int64, init=torch.zeros(8, dtype=torch.int64)), Guarded((1,)), \
        Guarded((3,), torch.int64, init=torch.zeros(3, dtype=torch.int64)), Guarded((5, 4))
    rollout.rollout_loss(rec0.t, 0.37, loss0.t, log0.t)
    rollout.rollout_loss(rec0.t, 0.37, loss0.t, log0.t)
    rollout.rollout_ce_bwd(x[:2], y[:2], rec0.t, 0.37, None, rr.IGNORE, dl0.t[:2])
    torch.cuda.synchronize()
    assert bits(loss0.t).tolist() == [0] and struct.unpack(rollout.LOG_FMT, log0.t.cpu().numpy().tobytes()) == (0.0, 2, 0)
    assert bool((dl0.t[:2, [0, 2, 3]].cpu() == 0).all()) and bits(dl0.t[2:]).unique().tolist() == [NAN_BITS]
    rec0.intact("the empty record")


def test_refusals_leave_every_fill_intact():
    L = _lib.lib()
    x, y = rr.make_steps(7, 9, 1, 0.0, "none", 1, DEV)[0]
    rec, nll, dl, loss = Guarded((8,), torch.int64), Guarded((7,)), Guarded((7, 9)), Guarded((1,))
    p = lambda t: t.data_ptr()
    calls = [lambda: L.etp_rollout_ce_fwd(p(x), p(y), 0, 9, rr.IGNORE, p(rec.t), p(nll.t), None),
             lambda: L.etp_rollout_ce_fwd(p(x), p(y), 7, 9, rr.IGNORE, p(rec.t) + 4, p(nll.t), None),
             lambda: L.etp_rollout_ce_fwd(p(x), p(y), 7, 9, rr.IGNORE, p(rec.t), p(rec.t) + 8, None),
             lambda: L.etp_rollout_loss(p(rec.t), 1.0, p(rec.t), None, None),
             lambda: L.etp_rollout_loss(p(rec.t), 1.0, p(loss.t) + 2, None, None),
             lambda: L.etp_rollout_loss(None, 1.0, p(loss.t), None, None),
             lambda: L.etp_rollout_ce_bwd(p(x), p(y), 7, 0, rr.IGNORE, p(rec.t), 1.0, None, p(dl.t), None),
             lambda: L.etp_rollout_ce_bwd(p(x), None, 7, 9, rr.IGNORE, p(rec.t), 1.0, None, p(dl.t), None),
             lambda: L.etp_rollout_ce_bwd(p(x), p(y), 7, 9, rr.IGNORE, p(rec.t), 1.0, None, p(dl.t) + 2, None)]
    for i, c in enumerate(calls):
        assert c() == -1, i
    torch.cuda.synchronize()
    for g in (rec, nll, dl, loss):
        g.intact("refusals")


# ---- RolloutLoss ---------------------------------------------------------------------------------------------------------------------------
def test_rollout_loss_gradients_are_the_direct_launches_bits():
    w = 0.37
    steps = rr.make_steps(17, 65, 3, 0.0, "some", 21, DEV)
    loss_d, dls_d, rec_d, _ = run_direct(steps, w, name="direct")
    leaves = [x.clone().requires_grad_(True) for x, _ in steps]
    rl, log = rollout.RolloutLoss(DEV), rollout.RolloutLog(DEV)
    for x, (_, y) in zip(leaves, steps):
        rl.add(x, y)
    total = rl.total(w, log=log)
    assert total.requires_grad and total.dim() == 0
    (total * 1.0).backward()
    assert torch.equal(bits(total), bits(loss_d.reshape(())))
    for x, d in zip(leaves, dls_d):
        assert torch.equal(bits(x.grad), bits(d))
    assert rl.record() == rec_d and log.read_raw() == (float(total.detach()), 1, 0) and log.read() == float(total.detach())
    with pytest.raises(RuntimeError):
        rl.add(leaves[0], steps[0][1])
    with pytest.raises(RuntimeError):
        rl.total(w)
    # a host list of labels and a scaled upstream gradient; reset() starts the next rollout with a fresh record
    rl.reset()
    x = steps[0][0].clone().requires_grad_(True)
    rl.add(x, steps[0][1].tolist())
    (0.5 * rl.total(w)).backward()
    rr.check_dlogits("upstream 0.5 through autograd", [x.grad], [(steps[0][0].cpu(), steps[0][1].cpu())], w, upstream=0.5)
    assert rl.record()["n_steps"] == 1
    # under no_grad nothing is kept and no graph is built
    rl.reset()
    with torch.no_grad():
        rl.add(leaves[0], steps[0][1])
        out = rl.total(w)
    assert not out.requires_grad and rl._steps == [] and rl._inputs == []
    with pytest.raises(ValueError):
        rollout.RolloutLoss(DEV).add(leaves[0], steps[1][1])


def test_rollout_loss_replays_the_recording_without_a_device_to_host_copy(monkeypatch):
    z, meta, steps = rr.load_fixture()
    w = meta["cfg"]["ml_weight"]
    copies = []
    for fn in ("cpu", "tolist", "item", "numpy", "nonzero"):
        real = getattr(torch.Tensor, fn)

        def counted(self, *a, _real=real, _fn=fn, **k):
            if self.is_cuda:
                copies.append(_fn)
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, fn, counted)
    leaves = [x.to(DEV).requires_grad_(True) for x, _ in steps]
    labels = [y.to(DEV) for _, y in steps]
    rl, log = rollout.RolloutLoss(DEV), rollout.RolloutLog(DEV)
    for x, y in zip(leaves, labels):
        rl.add(x, y)
    total = rl.total(w, log=log)
    total.backward()
    assert copies == [], f"device-to-host copies before record(): {copies}"
    rec = rl.record()
    assert copies == ["cpu"], copies
    monkeypatch.undo()
    assert (rec["n_actions"], rec["n_counted"], rec["n_steps"], rec["n_nonfinite"]) == (13, 12, 5, 0)
    r = rr.check_loss("fixture", total, steps, w)
    rr.check_dlogits("fixture", [x.grad for x in leaves], steps, w)
    rr.check_record("fixture", rec, steps)
    # against the reference's own fp32 results: its fp32 error is added to the bound
    bl, bd = rr.fixture_fp32_bounds(r, w)
    t64 = lambda v: torch.tensor(v, dtype=F64)
    rr.within(("fixture", "loss vs fp32 recording"), total.detach().cpu().reshape(()), t64(float(z["loss_f32"])), t64(rr.loss_bound(r, w) + bl))
    for t, (x, b, e) in enumerate(zip(leaves, rr.dlogits_bounds(r), bd)):
        rr.within(("fixture", "dlogits vs fp32 recording"), x.grad.cpu(), torch.from_numpy(z[f"dlogits_f32_{t}"]), b + e)


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------
S_IMG, MAX_LEN, N_ENVS, ML_WEIGHT = 64, 4, 3, 0.75
STARTS = [[0.0, 0.0, 0.0], [20.0, 0.0, 0.0], [40.0, 0.0, 0.0]]
GOALS = [[0.5, 0.0, -0.5], [20.0, 0.0, -3.0], [40.0, 0.0, -40.0]]          # within 1.5 at once; a step or two away; out of reach
_OBS = {}


def make_obs(slot, step, pos):
    """one environment's observation: token ids of the slot, 12 rgb and 12 depth views drawn from (slot, step), in the rollout's key
    order (rgb, depth, rgb_30.0, depth_30.0, ...)"""
    from tests import clip_ref as cr
    from tests import depth_ref as dr
    if (slot, step) not in _OBS:
        images, depth = cr.make_images(12, S_IMG, 100 * slot + step + 1), dr.make_depth(10 * slot + step, 12, S_IMG)
        g = np.random.default_rng(slot)
        ids = g.integers(2, 1000, 10)
        ids[8 - slot:] = 0
        obs = {"instruction": torch.from_numpy(ids.astype(np.int64))}
        for a in range(12):
            suffix = "" if a == 0 else f"_{a * 30.0}"
            obs["rgb" + suffix], obs["depth" + suffix] = images[a].contiguous(), depth[a].contiguous()
        _OBS[(slot, step)] = obs
    return _OBS[(slot, step)]


def obs_to_batch(observations):
    return {k: torch.stack([o[k] for o in observations]).to(DEV) for k in observations[0]}


@pytest.fixture(scope="module")
def world():
    from etpnav_amd import clip as cl
    from etpnav_amd import depth as dp
    from etpnav_amd import waypoint as wp
    from etpnav_amd.policy import ETP
    from tests import clip_ref as cr
    from tests import depth_ref as dr
    from tests import waypoint_ref as wr
    with torch.random.fork_rng(devices=[torch.cuda.current_device()]):          # the process's random streams stay as the other files find them
        torch.manual_seed(3)
        net = ETP(model_config=SimpleNamespace(task_type="r2r"), dtype=torch.float32, device=DEV)
    _, bp, blocks = dr.ALL_CASES[0]
    net.rgb_encoder = cl.CLIPEncoder(device=DEV, dtype=torch.float32, image_size=S_IMG, layers=2)
    net.rgb_encoder.load_state_dict(cr.make_weights(S_IMG, 2, 3), strict=True)
    net.depth_encoder = dp.DepthEncoder(device=DEV, dtype=torch.float32, image_size=S_IMG, base_planes=bp, blocks=blocks)
    net.depth_encoder.load_state_dict(dr.make_weights(S_IMG, bp, blocks, 3), strict=True)
    pred = wp.BinaryDistPredictorTRM(device=DEV, dtype=torch.float32)
    pred.load_state_dict(wr.make_weights(2), strict=True)
    pred.eval()
    net.eval()                                # no dropout: the two routes are compared bit for bit
    cfg = rollout.RolloutConfig(max_len=MAX_LEN, waypoint_aug=False, hidden=768)
    uniforms = torch.rand(MAX_LEN, N_ENVS, 2, generator=torch.Generator().manual_seed(8)).numpy()
    uniforms[..., 1] = 0.0                    # u1 <= sample_ratio: the teacher's action is taken, so the goals script the episodes
    return SimpleNamespace(net=net, pred=pred, cfg=cfg, uniforms=[u for u in uniforms])


def new_envs():
    return rr.ScriptedEnvs(STARTS, GOALS, make_obs=make_obs)


def grads_of(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def sliced_for(envs, table):
    class U:
        def __getitem__(self, stepk):
            return np.ascontiguousarray(table[stepk][:envs.num_envs])
    return U()


@pytest.mark.parametrize("fuse", [False, True], ids=["reference pano inputs", "fused pano inputs"])
def test_driver_equals_the_hand_composed_rollout(world, fuse):
    net = world.net
    try:
        net.fuse_pano_inputs = fuse
        net.zero_grad()
        envs_r = new_envs()
        loss_r, trace_r = rr.hand_composed_rollout(net, world.pred, envs_r, world.cfg, obs_to_batch, DEV, ML_WEIGHT, 0.5,
                                                   sliced_for(envs_r, world.uniforms), random.Random(4))
        loss_r.backward()
        grads_r = grads_of(net)
        # the script makes the environments finish at different steps: asserted on the reference alone
        assert len({len(e["slots"]) for e in trace_r}) >= 2 and len(trace_r) >= 2, [e["slots"] for e in trace_r]
        assert trace_r[0]["teacher"][0] == 0 and trace_r[0]["env_actions"][0]["action"]["act"] == 0 and trace_r[1]["slots"][0] != 0

        net.zero_grad()
        envs_d, trace_d, done = new_envs(), [], []
        drv = rollout.RolloutDriver(net, world.pred, envs_d, world.cfg, obs_to_batch, DEV, rng=random.Random(4), trace=trace_d,
                                    on_done=lambda slot, ep, info, view: done.append(slot))
        loss_d = drv.rollout("train", ML_WEIGHT, 0.5, uniforms=sliced_for(envs_d, world.uniforms))
        loss_d.backward()
        drv.check()
        grads_d = grads_of(net)

        assert len(trace_d) == len(trace_r) and sorted(done) == [0, 1, 2] and len(done) == 3
        steps = []
        for a, b in zip(trace_d, trace_r):
            k = a["stepk"]
            assert (a["slots"], a["cur_vp"], a["teacher"], a["a_t"]) == (b["slots"], b["cur_vp"], b["teacher"], b["a_t"]), k
            assert torch.equal(bits(a["nav_logits"]), bits(b["nav_logits"])), f"step {k}: nav_logits differ"
            for x, y in zip(a["env_actions"], b["env_actions"]):
                assert sorted(x["action"]) == sorted(y["action"]), k
                for key, v in x["action"].items():
                    if key == "back_path":
                        assert (v is None) == (y["action"][key] is None) and [p[0] for p in v or []] == [p[0] for p in y["action"][key] or []], k
                    elif isinstance(v, np.ndarray):
                        assert v.tobytes() == np.asarray(y["action"][key]).tobytes(), (k, key)
                    else:
                        assert v == y["action"][key], (k, key)
            steps.append((a["nav_logits"].float().cpu(), torch.tensor(a["teacher"], dtype=torch.int64)))
        rr.check_loss(f"driver fuse={fuse}", loss_d, steps, ML_WEIGHT)
        ref64 = rr.reference(steps, ML_WEIGHT)["loss"]
        assert abs(float(loss_r) - ref64) <= 1e-5 * max(1.0, abs(ref64))              # torch's fp32 loss of the hand-composed route, loosely
        assert set(grads_d) == set(grads_r) and grads_d
        for k in grads_r:
            tol = 1e-4 * max(1.0, float(grads_r[k].abs().max()))
            assert float((grads_d[k] - grads_r[k]).abs().max()) <= tol, k
        assert any(float(g.abs().max()) > 0 for g in grads_d.values())
    finally:
        net.fuse_pano_inputs = False


def test_eval_builds_no_graph_and_calls_on_done_once_per_episode(world):
    net, done = world.net, []
    envs = new_envs()
    trace = []
    drv = rollout.RolloutDriver(net, world.pred, envs, world.cfg, obs_to_batch, DEV, trace=trace,
                                on_done=lambda slot, ep, info, view: done.append((slot, ep.episode_id, len(view.node_pos))))
    assert drv.rollout("eval") is None
    assert sorted(d[0] for d in done) == [0, 1, 2] and len(done) == 3 and all(d[2] >= 1 for d in done)
    assert all(not e["nav_logits"].requires_grad and e["teacher"] is None for e in trace) and drv.loss is None
    assert envs.num_envs == 0 and 1 <= len(trace) <= MAX_LEN


def test_two_iterations_of_train_interval_move_the_parameters(world):
    from etpnav_amd.optim import FusedAdamW
    net = world.net
    before = {k: p.detach().clone() for k, p in net.vln_bert.named_parameters()}
    envs = new_envs()
    drv = rollout.RolloutDriver(net, world.pred, envs, world.cfg, obs_to_batch, DEV, rng=random.Random(4), generator=torch.Generator(DEV).manual_seed(1))
    opt = FusedAdamW(net.vln_bert, lr=1e-3)
    losses = []
    real = rollout.RolloutLoss.total

    def keep(self, ml_weight, log=None):
        out = real(self, ml_weight, log=log)
        losses.append(out.detach())
        return out
    try:
        rollout.RolloutLoss.total = keep
        logs = drv.train_interval(2, ML_WEIGHT, 0.5, opt)
    finally:
        rollout.RolloutLoss.total = real
        net.eval()
    assert len(losses) == 2 and envs.round == 1
    vals = [float(l) for l in losses]
    assert logs["IL_loss"] == (vals[0] + vals[1]) / 2 and all(np.isfinite(vals))          # two fp32 values: their double sum is exact
    moved = [k for k, p in net.vln_bert.named_parameters() if not torch.equal(p.detach(), before[k])]
    assert moved, "no parameter moved"
