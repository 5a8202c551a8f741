"""etp_traj_nodes_fwd / etp_traj_nodes_bwd (csrc/traj_batch.hip) on the MI355X: the trajectory node features straight from the integer
tables, against etp_gather_sum over graph_inputs.pack_traj_csr of the same batch (bit for bit) and the float64 restatement of
tests/traj_nodes_ref.py (within gam(n) * sum |w x|, n the terms of the row: one rounding per fused multiply-add, no multiplier).

Operators: H in {256, 512, 768} x B in {1, 3, 8} x V in {1, 5, 36, 39}.  B = 1 is one random sample of 70 steps (a second trip of the
lane loops over steps) with candidate counts from {0, 1, 5, 64} (every lane a slot); B = 3 the crafted samples of traj_nodes_ref.crafted
(a viewpoint visited twice, a ghost seen from three steps and twice within one, slots at and beyond view_len, a candidate visited later,
gmap_len = 1, both node orders of (A) and (B)); B = 8 the four crafted samples and four random ones of 1, 2, 5 and 21 steps.  G is the
batch maximum + 2 (padding rows).  Operands carry row scales 2^-10 .. 2^3; outputs start as payload NaNs inside guarded buffers; inputs
are unchanged; a second run is bit-identical.  Each device flag is planted once; refusals leave the fill intact.

Through the steps: PlannerStep on make_sap_batch (B = 4, T = 3, ragged; fp32 and bf16; eval and dropout="config") and MlmStep give the same
gimg, logits and loss bits on both routes (the MLM loss is a sum of float atomics, one per masked token: held to the bound of that sum),
and d_pano is etp_gather_sum(csr_b) of the step's own d_gimg; load_batch takes a batch of another Kmax; SapBatches on the fixture corpus feeds a step with pack_traj_csr patched to raise."""
import copy
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd import graph_inputs as gi  # noqa: E402
from etpnav_amd import pretrain_data as pdata  # noqa: E402
from tests import move_ref as mr  # noqa: E402
from tests import traj_nodes_ref as tr  # noqa: E402

DEV = "cuda"
TABLES = ("step_off", "step_vp", "view_lens", "cand_count", "cand_vp", "gmap_id", "gmap_len")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pick(traj, which):
    return {k: [traj[k][i] for i in which] for k in traj}


def make_traj(B, V, seed):
    rng = np.random.RandomState(seed)
    if B == 1:
        return tr.random_traj(rng, 1, V, [70], [0, 1, 5, 64], names_per_sample=12)
    if B == 3:
        return pick(tr.crafted(V), [0, 1, 2])
    return tr.concat(tr.crafted(V), tr.random_traj(rng, 4, V, [1, 2, 5, 21], [0, 1, 5, 64], names_per_sample=10))


class Case:
    def __init__(self, H, B, V, seed=0):
        self.traj = make_traj(B, V, seed + 7 * V + B)
        self.H, self.B, self.V = H, B, V
        self.G = max(len(g) for g in self.traj["gmap_vpids"]) + 2
        self.tb = tr.tables(self.traj, self.G)
        self.R, self.K = len(self.tb["step_vp"]), self.tb["cand_vp"].shape[1]
        rng = np.random.RandomState(seed + 1)
        self.pano, self.dg = tr.scaled_rows(rng, self.R * V, H), tr.scaled_rows(rng, B * self.G, H)
        t = self.traj
        f, b = gi.pack_traj_csr(t["traj_vp_lens"], t["traj_vpids"], t["traj_cand_vpids"], t["gmap_vpids"], V, self.G)
        self.csr_f, self.csr_b = tuple(x.to(DEV) for x in f), tuple(x.to(DEV) for x in b)

    def upload(self, tb=None):
        d = {k: dev(v) for k, v in (tb or self.tb).items()}
        d["pano"], d["dg"] = dev(self.pano), dev(self.dg)
        return d

    def gather(self, src, csr, n_out):
        out = torch.empty(n_out, self.H, dtype=torch.float32, device=DEV)
        rc = _lib.lib().etp_gather_sum(_lib.ETP_F32, src.data_ptr(), csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), out.data_ptr(),
                                       n_out, self.H, 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _lib.lib().etp_last_error()
        return out


class Outputs:
    def __init__(self, c):
        self.gimg, self.dpano = mr.guarded((c.B * c.G, c.H)), mr.guarded((c.R * c.V, c.H))
        self.g_st = mr.guarded(((c.B * c.G + c.R) * 4,), torch.uint8)
        self.st = self.g_st.t.view(torch.int32)
        self.n_nodes = c.B * c.G

    def check(self, name):
        for g in (self.gimg, self.dpano, self.g_st):
            g.check(name)


def launch(c, d, out, which="both", **override):
    a = dict(B=c.B, R=c.R, V=c.V, Kmax=c.K, G=c.G, H=c.H)
    a.update(override)
    L, s = _lib.lib(), torch.cuda.current_stream().cuda_stream
    tabs = [d[k].data_ptr() for k in TABLES]
    dims = [a[k] for k in ("B", "R", "V", "Kmax", "G", "H")]
    rc = []
    if which in ("both", "fwd"):
        rc.append(L.etp_traj_nodes_fwd(d["pano"].data_ptr(), *tabs, *dims, out.gimg.t.data_ptr(), out.st.data_ptr(), s))
    if which in ("both", "bwd"):
        rc.append(L.etp_traj_nodes_bwd(d["dg"].data_ptr(), *tabs, *dims, out.dpano.t.data_ptr(), out.st.data_ptr() + 4 * out.n_nodes, s))
    torch.cuda.synchronize()
    return rc


def within(name, got, ref, mag, terms):
    """|got - ref| <= gam(n) * sum |w x| per element, n the row's terms; a row without terms is exact zeros"""
    bound = tr.gam(terms.astype(np.float64))[:, None] * mag
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if (bound > 0).any() else 0.0
    print(f"{name}: worst err/bound {worst:.3f}, rows with terms {int((terms > 0).sum())} of {len(terms)}")
    assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} elements beyond gam(n) * sum|w x| (worst ratio {worst:.3f})"


GRID = [(H, B, V) for H in (256, 512, 768) for B in (1, 3, 8) for V in (1, 5, 36, 39)]


@pytest.mark.parametrize("H,B,V", GRID, ids=[f"H{H}-B{B}-V{V}" for H, B, V in GRID])
def test_kernels_equal_gather_sum_over_the_csr_and_lie_within_the_fp64_bound(H, B, V):
    c = Case(H, B, V)
    name = f"H{H} B{B} V{V} G{c.G} R{c.R} K{c.K}"
    if B == 1:
        assert c.R == 70 and c.K == 64
    d = c.upload()
    keep = {k: v.clone() for k, v in d.items()}
    out = Outputs(c)
    assert launch(c, d, out) == [0, 0], _lib.lib().etp_last_error()
    out.check(name)
    assert not out.st.any(), out.st.cpu().tolist()
    mr.exact(name + " gmap_img_fts vs etp_gather_sum", out.gimg.t, c.gather(d["pano"], c.csr_f, B * c.G))
    mr.exact(name + " d_pano vs etp_gather_sum", out.dpano.t, c.gather(d["dg"], c.csr_b, c.R * V))
    ref, st, mag, terms = tr.forward(c.pano, c.tb, V)
    refb, stb, magb, termsb = tr.backward(c.dg, c.tb, V)
    assert not st.any() and not stb.any()
    within(name + " fwd", out.gimg.t.cpu().numpy(), ref, mag, terms)
    within(name + " bwd", out.dpano.t.cpu().numpy(), refb, magb, termsb)
    if B >= 3:
        assert (termsb == 2).any() and (termsb == 0).any() and (terms == 0).any()
    again = Outputs(c)
    assert launch(c, d, again) == [0, 0]
    mr.exact(name + " fwd second run", again.gimg.t, out.gimg.t)
    mr.exact(name + " bwd second run", again.dpano.t, out.dpano.t)
    for k, v in keep.items():
        mr.exact(name + f" {k} unchanged", d[k], v)


def test_crafted_samples_zero_rows_and_the_revisited_step():
    """what the contract says in words, read off the device result: the earlier visit's rows and every row beyond view_len get exact zero
    gradients, [stop] / padding / a ghost only seen beyond the valid views are exact zero rows"""
    c = Case(256, 3, 5)
    out = Outputs(c)
    assert launch(c, c.upload(), out) == [0, 0]
    gimg, dp = out.gimg.t.cpu().view(c.B, c.G, c.H), out.dpano.t.cpu().view(c.R, c.V, c.H)
    assert not dp[1].any()                                        # sample 0 visits "b" at steps 1 and 3: step 1 feeds nothing
    assert dp[0, 0].any() and dp[0, 2].any() and dp[3, 0].any()   # the ghost's two slots of step 0; the last visit of "b"
    for b in range(c.B):
        ln = len(c.traj["gmap_vpids"][b])
        assert not gimg[b, 0].any() and not gimg[b, ln:].any()
    y = c.traj["gmap_vpids"][1].index("y")
    assert not gimg[1, y].any() and gimg[1, 1].any()             # "y": one slot, beyond view_len 1 of its step
    lens = np.asarray(c.tb["view_lens"])
    for r in range(c.R):
        assert not dp[r, lens[r]:].any()
    assert torch.isfinite(gimg).all() and torch.isfinite(dp).all()


def test_each_device_flag_keeps_its_rows_fill_and_leaves_the_others_correct():
    c = Case(512, 8, 5)
    good = Outputs(c)
    assert launch(c, c.upload(), good) == [0, 0]
    off = c.tb["step_off"]
    plants = {"steps": ("step_off", c.B, c.R + 1, tr.ERR_STEPS, c.B - 1), "steps empty": ("step_off", c.B, int(off[c.B - 1]), tr.ERR_STEPS, c.B - 1),
              "count": ("cand_count", 1, c.K + 1, tr.ERR_COUNT, 0), "count -1": ("cand_count", int(off[1]), -1, tr.ERR_COUNT, 1),
              "views": ("view_lens", int(off[1]), c.V + 1, tr.ERR_VIEWS, 1), "views 0": ("view_lens", 0, 0, tr.ERR_VIEWS, 0),
              "len": ("gmap_len", 3, c.G + 1, tr.ERR_LEN, 3), "len 0": ("gmap_len", 0, 0, tr.ERR_LEN, 0)}
    for name, (key, at, value, flag, sample) in plants.items():
        tb = {k: v.copy() for k, v in c.tb.items()}
        tb[key][at] = value
        out = Outputs(c)
        fill_f, fill_b = out.gimg.t.clone(), out.dpano.t.clone()
        assert launch(c, c.upload(tb), out) == [0, 0], name
        out.check(name)
        _, want_f, _, _ = tr.forward(c.pano[:, :2], tb, c.V, np.float32)
        _, want_b, _, _ = tr.backward(c.dg[:, :2], tb, c.V, np.float32)
        st = out.st.cpu().numpy()
        assert st[:c.B * c.G].tolist() == want_f.tolist() and st[c.B * c.G:].tolist() == want_b.tolist(), name
        rows = torch.from_numpy(want_f != 0).to(DEV)
        steps = torch.from_numpy(np.repeat(want_b != 0, c.V)).to(DEV)
        # one sample's node rows and its steps ("steps empty": the last sample owns no step; its former steps belong to nobody)
        assert bool(steps.any()) and (want_f[want_f != 0] == flag).all() and (want_b[want_b != 0] == flag).all(), name
        assert rows.view(c.B, c.G)[sample].all() and int(rows.sum()) == c.G
        assert want_b.nonzero()[0].tolist() == list(range(int(off[sample]), int(off[sample + 1]))), name
        mr.exact(name + " flagged node rows keep the fill", out.gimg.t[rows], fill_f[rows])
        mr.exact(name + " other node rows", out.gimg.t[~rows], good.gimg.t[~rows])
        mr.exact(name + " flagged steps keep the fill", out.dpano.t[steps], fill_b[steps])
        mr.exact(name + " other steps", out.dpano.t[~steps], good.dpano.t[~steps])
    tb = {k: v.copy() for k, v in c.tb.items()}
    tb["gmap_id"][0, 5] = 2 ** 31 - 1                             # a listed node that nothing visits or names
    out = Outputs(c)
    fill_f = out.gimg.t.clone()
    assert launch(c, c.upload(tb), out) == [0, 0]
    st = out.st.cpu().numpy()
    assert st[5] == tr.ERR_NODE and st.sum() == tr.ERR_NODE
    keep = torch.ones(c.B * c.G, dtype=torch.bool, device=DEV)
    keep[5] = False
    mr.exact("node: the row keeps the fill", out.gimg.t[5], fill_f[5])
    mr.exact("node: other rows", out.gimg.t[keep], good.gimg.t[keep])
    # the backward has no such flag: the one slot that named "h" (step 2, view 1 of sample 0) no longer finds its node listed and keeps
    # only (A)'s term, one product rounded once; every other row is as before
    r = 2 * c.V + 1
    others = torch.ones(c.R * c.V, dtype=torch.bool, device=DEV)
    others[r] = False
    mr.exact("node: backward, other rows", out.dpano.t[others], good.dpano.t[others])
    want, stb, _, terms = tr.backward(c.dg, tb, c.V, np.float32)
    assert terms[r] == 1 and not stb.any() and not st[c.B * c.G:].any()
    mr.exact("node: backward, the slot's row", out.dpano.t[r].cpu(), torch.from_numpy(want[r]))


def test_refusals_leave_the_fill_intact():
    c = Case(256, 3, 5)
    d = c.upload()
    out = Outputs(c)
    fill = (out.gimg.buf.clone(), out.dpano.buf.clone(), out.g_st.buf.clone())
    for override in (dict(H=128), dict(H=640), dict(H=1024), dict(B=0), dict(R=0), dict(V=0), dict(G=0), dict(Kmax=0), dict(Kmax=65)):
        assert launch(c, d, out, **override) == [-1, -1], override
        assert b"etp_traj_nodes_bwd" in _lib.lib().etp_last_error()
    d2 = dict(d, pano=d["pano"].view(-1)[1:], dg=d["dg"].view(-1)[2:])          # 4- and 8-byte aligned only
    assert launch(c, d2, out) == [-1, -1]
    for got, want in zip((out.gimg.buf, out.dpano.buf, out.g_st.buf), fill):
        mr.exact("refusals", got, want)


def test_aggregate_gmap_features_takes_the_descriptors_and_builds_no_csr(monkeypatch):
    c = Case(256, 3, 5)
    t = c.traj
    x = dev(c.pano).view(c.R, c.V, c.H).requires_grad_(True)
    want = gi.aggregate_gmap_features(x, t["traj_vp_lens"], t["traj_vpids"], t["traj_cand_vpids"], t["gmap_vpids"], c.G)
    want.backward(dev(c.dg).view(c.B, c.G, c.H))
    gx, x.grad = x.grad, None
    td = gi.traj_descriptors(t, c.G, DEV)
    monkeypatch.setattr(gi, "pack_traj_csr", lambda *a, **k: (_ for _ in ()).throw(AssertionError("pack_traj_csr was called")))
    got = gi.aggregate_gmap_features(x, dev(c.tb["view_lens"]), None, None, None, c.G, traj_dev=td)
    got.backward(dev(c.dg).view(c.B, c.G, c.H))
    mr.exact("aggregate_gmap_features", got.detach(), want.detach())
    mr.exact("aggregate_gmap_features backward", x.grad, gx)
    assert gi.traj_status_message(td["status"].cpu().numpy(), c.B * c.G, c.G) is None


# ---- through the steps -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pretrain_case():
    from oracle.make_golden_pretrain import make_case
    return make_case()


def _model(cfg, P, dtype):
    from etpnav_amd.planner import GlocalTextPathNavCMT
    m = GlocalTextPathNavCMT(cfg.to_dict(), dtype=dtype, device=DEV)
    m.load_state_dict(dict(P), strict=True)
    return m.eval()


def _sap_batch(cfg, seed=77):
    from etpnav_amd.synthetic import make_sap_batch
    return make_sap_batch(cfg.vocab_size, cfg.image_feat_size, cfg.depth_feat_size, B=4, L=19, T=3, V=9, n_cand=4, seed=seed, ragged=True)


def _run(step):
    step.run_eager()
    torch.cuda.synchronize()
    return {k: getattr(step, k).clone() for k in ("gimg", "loss", "d_gimg", "d_pano") + (("logits",) if hasattr(step, "logits") else ())}


def _compare_routes(name, old, new, csr_step, H, loss_atomic_terms=0):
    """forward bits equal across the routes; the new route's d_pano is etp_gather_sum(csr_b) of its OWN d_gimg (the step's gradients
    pass through atomics and are not compared across runs).  loss_atomic_terms = Nm for the MLM loss: vocab_ce_kernel adds one
    non-negative term scale * nll per masked token to *loss with a float atomicAdd, so two runs of ONE route already differ by the
    order of Nm additions.  Each run is within gam(Nm - 1) * sum |terms| = gam(Nm - 1) * loss of the exact sum of the same terms
    (gimg, hence every term, is bit-equal), so the two lie within twice that of each other."""
    for k in ("gimg",) + (("logits",) if "logits" in old else ()) + (() if loss_atomic_terms else ("loss",)):
        mr.exact(f"{name}: {k}", new[k], old[k])
    if loss_atomic_terms:
        a, b = float(new["loss"].double()), float(old["loss"].double())
        bound = 2 * tr.gam(loss_atomic_terms - 1) * max(abs(a), abs(b))
        print(f"{name}: loss {a!r} against {b!r}, |difference| {abs(a - b):.3g}, bound {bound:.3g}")
        assert abs(a - b) <= bound, (name, a, b, bound)
    pb, xb, wb = csr_step.csr_b
    want = torch.empty_like(new["d_pano"])
    n = want.shape[0] * want.shape[1]
    assert _lib.lib().etp_gather_sum(_lib.ETP_F32, new["d_gimg"].data_ptr(), pb.data_ptr(), xb.data_ptr(), wb.data_ptr(), want.data_ptr(), n, H, 0,
                                     torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    mr.exact(f"{name}: d_pano", new["d_pano"], want)
    assert torch.isfinite(new["d_pano"]).all() and new["d_pano"].any()


@pytest.mark.parametrize("dropout", [None, "config"], ids=["eval", "dropout"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_planner_step_gives_the_same_bits_on_both_routes(pretrain_case, dtype, dropout):
    from etpnav_amd.step import PlannerStep
    cfg, P, _ = pretrain_case
    model = _model(cfg, P, dtype)
    batch = _sap_batch(cfg)
    old_step = PlannerStep(model, batch, dropout=dropout, drop_seed=5)
    new_step = PlannerStep(model, batch, dropout=dropout, drop_seed=5, traj_nodes=True)
    try:
        assert not old_step.traj_nodes and old_step.csr_f is not None and new_step.traj_nodes and new_step.csr_f is None
        old, new = _run(old_step), _run(new_step)
        _compare_routes(f"PlannerStep {dtype} {dropout}", old, new, old_step, cfg.hidden_size)
        new_step.check_traj()
        old_step.check_traj()
        # a second batch of the same shapes with another Kmax: one more slot at one step, naming a ghost the graph already lists
        b2 = dict(_sap_batch(cfg, seed=78))
        b2["traj"] = copy.deepcopy(b2["traj"])
        ghost = b2["traj"]["gmap_vpids"][1][-1]
        b2["traj"]["traj_cand_vpids"][1][0].append(ghost)
        k0 = int(new_step.traj_dev["Kmax"])
        old_step.load_batch(b2)
        new_step.load_batch(b2)
        assert int(new_step.traj_dev["Kmax"]) == k0 + 1
        _compare_routes(f"PlannerStep {dtype} {dropout} after load_batch", _run(old_step), _run(new_step), old_step, cfg.hidden_size)
        new_step.check_traj()
    finally:
        torch.cuda.synchronize()
        old_step.close()
        new_step.close()


def test_planner_step_switches_and_check_traj(pretrain_case, monkeypatch):
    from etpnav_amd.step import PlannerStep
    cfg, P, _ = pretrain_case
    model = _model(cfg, P, torch.float32)
    batch = _sap_batch(cfg)
    monkeypatch.setenv("ETP_TRAJ_NODES", "0")
    off = PlannerStep(model, batch, traj_nodes=True)               # the switch is read at construction and wins
    monkeypatch.delenv("ETP_TRAJ_NODES")
    assert not off.traj_nodes and off.csr_f is not None
    off.close()
    step = PlannerStep(model, batch, traj_nodes=True)
    try:
        step.traj_dev["gmap_id"][2, 1] = 2 ** 30                   # a listed node that nothing visits or names
        step.run_eager()
        with pytest.raises(_lib.EtpError, match=r"\(sample 2, node 1\): 32"):
            step.check_traj()
    finally:
        torch.cuda.synchronize()
        step.close()


def test_mlm_step_gives_the_same_bits_on_both_routes(pretrain_case):
    from etpnav_amd.pretrain import MlmStep
    cfg, P, mlm_batch = pretrain_case
    model = _model(cfg, P, torch.float32)
    old_step, new_step = MlmStep(model, mlm_batch), MlmStep(model, mlm_batch, traj_nodes=True)
    try:
        assert not old_step.traj_nodes and new_step.traj_nodes
        _compare_routes("MlmStep", _run(old_step), _run(new_step), old_step, cfg.hidden_size, loss_atomic_terms=new_step.Nm)
        new_step.check_traj()
    finally:
        torch.cuda.synchronize()
        old_step.close()
        new_step.close()


def test_sap_batches_feed_a_step_without_pack_traj_csr(pretrain_case, monkeypatch):
    """the native loader's TrajBatch: exactly the old keys, the descriptor tables beside them, and a PlannerStep that builds no CSR"""
    from etpnav_amd.features import FeatureStore, write_flat_pack
    from etpnav_amd.step import PlannerStep
    from tests import pretrain_data_ref as ref
    cfg, P, _ = pretrain_case
    c = ref.corpus()
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as td:                      # the fixture corpus over a store of the model's widths
        write_flat_pack(os.path.join(td, "img.etpf"), ((k, rng.standard_normal((36, cfg.image_feat_size)).astype(np.float32)) for k in c["keys"]))
        write_flat_pack(os.path.join(td, "dep.etpf"), ((k, rng.standard_normal((36, cfg.depth_feat_size)).astype(np.float32)) for k in c["keys"]))
        store = FeatureStore(os.path.join(td, "img.etpf"), os.path.join(td, "dep.etpf")).to_device(DEV)
    graphs = pdata.NavGraphs.from_connectivity(ref.js("connectivity")).to_device(DEV)
    annos = [dict(a, instr_encoding=[101] + [1000 + t % 1000 for t in a["instr_encoding"][1:-1]] + [102]) for a in c["annos"]]
    index = pdata.R2RTextPathIndex([annos], store, c["cands"], graphs, cfg.image_feat_size, cfg.depth_feat_size, 16)
    sap = pdata.SapBatches(index, 4, np.random.default_rng(3), DEV)
    samples = [tuple(x) for x in ref.js("samples")][:4]
    batch = sap.batch(samples)
    sap.check()
    assert isinstance(batch, pdata.TrajBatch) and set(batch) == set(ref.expected("sap_all")) and "traj_dev" not in batch
    td_ = batch.traj_dev
    tb = {k: td_[k].cpu().numpy() for k in gi.TRAJ_TABLES}
    G = batch["gmap_step_ids"].shape[1]
    mine = {k: gi.traj_descriptors(batch["traj"], G, "cpu")[k].numpy() for k in gi.TRAJ_TABLES}
    for b, ln in enumerate(tb["gmap_len"]):                        # the staging buffer pads gmap_idx with zeros; nothing reads them
        tb["gmap_id"][b, ln:] = -1
    assert tr.same_up_to_renaming(tb, mine) and td_["Kmax"] == tb["cand_vp"].shape[1]
    model = _model(cfg, P, torch.float32)
    old_step = PlannerStep(model, batch, traj_nodes=False)
    monkeypatch.setattr(gi, "pack_traj_csr", lambda *a, **k: (_ for _ in ()).throw(AssertionError("pack_traj_csr was called")))
    new_step = PlannerStep(model, batch)                           # default: the tables whenever the batch carries them
    try:
        assert new_step.traj_nodes and new_step.traj_dev is td_ and not old_step.traj_nodes
        old, new = _run(old_step), _run(new_step)
        _compare_routes("SapBatches", old, new, old_step, cfg.hidden_size)
        new_step.check_traj()
        assert np.isfinite(float(new["loss"])) and float(new["loss"]) > 0
        again = sap.batch(samples)
        new_step.load_batch(again)                                 # by reference: the new batch's tables
        assert new_step.traj_dev is again.traj_dev
        mr.exact("SapBatches after load_batch", _run(new_step)["gimg"], new["gimg"])
    finally:
        torch.cuda.synchronize()
        old_step.close()
        new_step.close()
