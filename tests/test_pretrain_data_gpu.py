"""etp_traj_views / etp_traj_pair_dists (csrc/traj_batch.hip) and the native loaders of etpnav_amd/pretrain_data.py on the MI355X.

Operators, bit for bit against tests/pretrain_data_ref.py, every output inside NaN / 0xFF-filled guarded buffers, a second run identical:
  etp_traj_views       R in {1, 3, 13} x (P, F_img, ld_img, F_dep, ld_dep) in {(36, 768, 768, 128, 128), (36, 16, 24, 8, 8),
                       (36, 260, 260, no depth), (5, 16, 16, 8, 12)}, k cycling through {0, 1, 5, Kmax = 7} with all candidates in one view
                       (length k + P - 1 > P), distinct views and repeated views, plus Kmax = 40 with every view a candidate; V = the batch
                       maximum and maximum + 3.  Each malformed condition keeps the fill for that step only; refusals leave everything intact.
  etp_traj_pair_dists  B in {1, 3, 8} x G in {1, 2, 9, 33, 70}, two scans of different n, asymmetric tables; one out-of-range index flagged.
End to end on tests/golden/pretrain_batch_small.npz: SapBatches / MlmBatches on the recorded sample choices give every tensor of the REAL
sap_collate / mlm_collate recording bit for bit; one PretrainDriver.train_step each for 'sap' and 'mlm' off the native loaders returns a
finite loss."""
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from etpnav_amd import _lib  # noqa: E402
from etpnav_amd import pretrain_data as pdata  # noqa: E402
from etpnav_amd.features import FeatureStore, write_flat_pack  # noqa: E402
from tests import move_ref as mr  # noqa: E402
from tests import pretrain_data_ref as ref  # noqa: E402

DEV = "cuda"
DIMS = [(36, 768, 768, 128, 128), (36, 16, 24, 8, 8), (36, 260, 260, None, None), (5, 16, 16, 8, 12)]
N_ROWS = 6


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def view_case(R, dims, Kmax=7, every_view=False, seed=0):
    """host inputs of etp_traj_views: small-integer features (every element of a store distinct per row), crafted candidate tables"""
    P, Fi, ldi, Fd, ldd = dims
    rng = np.random.default_rng(seed + 131 * R + P)
    img = rng.integers(-30000, 30000, (N_ROWS, P, ldi)).astype(np.float32)
    dep = None if Fd is None else rng.integers(-30000, 30000, (N_ROWS, P, ldd)).astype(np.float32)
    row = rng.integers(0, N_ROWS, R).astype(np.int32)
    row[0] = N_ROWS - 1
    count, view = np.zeros(R, np.int32), rng.integers(0, P, (R, Kmax)).astype(np.int32)        # beyond k: in range, never used
    for r in range(R):
        k = Kmax if every_view else [Kmax, 5, 1, 0][r % 4]
        count[r] = k
        if every_view:
            view[r, :P] = rng.permutation(P)
        elif r % 3 == 0:
            view[r, :k] = rng.integers(0, P)                     # all candidates in one view
        elif r % 3 == 1 and k <= P:
            view[r, :k] = rng.permutation(P)[:k]
    loc = rng.standard_normal((R, Kmax, 4)).astype(np.float32)
    tab = rng.standard_normal((P, 4)).astype(np.float32)
    lens = [int(count[r]) + P - len(set(view[r, :count[r]].tolist())) for r in range(R)]
    return {"img": img, "dep": dep, "row": row, "count": count, "view": view, "loc": loc, "tab": tab, "lens": lens, "dims": dims}


class ViewOutputs:
    def __init__(self, R, V, Fi, Fd):
        self.f = {"rgb_fts": mr.guarded((R, V, Fi)), "loc_fts": mr.guarded((R, V, 4))}
        if Fd is not None:
            self.f["dep_fts"] = mr.guarded((R, V, Fd))
        self.g_nav, self.nav = mr.guarded_i64((R, V))
        self.g_len, self.lens = mr.guarded_i64((R,))
        self.g_st = mr.guarded((R * 4,), torch.uint8)
        self.st = self.g_st.t.view(torch.int32)

    def guards(self):
        return list(self.f.values()) + [self.g_nav, self.g_len, self.g_st]

    def numpy(self):
        out = {k: g.t.cpu().numpy() for k, g in self.f.items()}
        out.update(nav_types=self.nav.cpu().numpy(), view_lens=self.lens.cpu().numpy(), status=self.st.cpu().numpy())
        return out


def launch_views(d, c, V, out, **override):
    P, Fi, ldi, Fd, ldd = c["dims"]
    a = dict(R=len(c["row"]), V=V, Kmax=c["view"].shape[1], P=P, F_img=Fi, ld_img=ldi, F_dep=Fd or 0, ld_dep=ldd or 0, N=N_ROWS)
    a.update(override)
    dp = lambda k: None if d[k] is None else d[k].data_ptr()
    rc = _lib.lib().etp_traj_views(dp("img"), dp("dep"), dp("row"), dp("count"), dp("view"), dp("loc"), dp("tab"), a["R"], a["V"], a["Kmax"],
                                   a["P"], a["F_img"], a["ld_img"], a["F_dep"], a["ld_dep"], a["N"], out.f["rgb_fts"].t.data_ptr(),
                                   out.f["dep_fts"].t.data_ptr() if "dep_fts" in out.f else None, out.f["loc_fts"].t.data_ptr(),
                                   out.nav.data_ptr(), out.lens.data_ptr(), out.st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def on_device(c):
    return {k: None if c[k] is None else dev(c[k]) for k in ("img", "dep", "row", "count", "view", "loc", "tab")}


def same(name, got, want):
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, (name, k, got[k].dtype, v.dtype, got[k].shape, v.shape)
        assert got[k].tobytes() == v.tobytes(), f"{name}: {k} differs in {int((got[k].view(np.uint8) != v.view(np.uint8)).sum())} bytes"


VIEW_CASES = [(R, d, 7, False) for R in (1, 3, 13) for d in DIMS] + [(3, DIMS[1], 40, True)]


@pytest.mark.parametrize("R,dims,Kmax,every", VIEW_CASES, ids=[f"R{R}-P{d[0]}-F{d[1]}of{d[2]}-D{d[3]}of{d[4]}-K{K}" for R, d, K, _ in VIEW_CASES])
def test_traj_views_against_the_restatement(R, dims, Kmax, every):
    c = view_case(R, dims, Kmax, every)
    d = on_device(c)
    keep = {k: v.clone() for k, v in d.items() if v is not None}
    assert every or R < 3 or max(c["lens"]) > dims[0]          # all candidates in one view: longer than the panorama
    for V in (max(c["lens"]), max(c["lens"]) + 3):
        name = f"R{R} {dims} K{Kmax} V{V}"
        want = ref.traj_views(c["img"], c["dep"], c["row"], c["count"], c["view"], c["loc"], c["tab"], V, dims[1], dims[3])
        assert not want["status"].any() and want["view_lens"].tolist() == c["lens"]
        out = ViewOutputs(R, V, dims[1], dims[3])
        assert launch_views(d, c, V, out) == 0, _lib.lib().etp_last_error()
        for g in out.guards():
            g.check(name)
        got = out.numpy()
        same(name, got, want)
        again = ViewOutputs(R, V, dims[1], dims[3])
        assert launch_views(d, c, V, again) == 0
        same(name + " second run", again.numpy(), got)
        for k, v in keep.items():
            mr.exact(name + f" {k} unchanged", d[k].cpu(), v.cpu())


def test_traj_views_malformed_steps_keep_the_fill_and_leave_the_others_correct():
    dims = DIMS[1]
    c = view_case(6, dims, seed=3)
    c["count"][:] = [1, 8, 2, 1, 7, -1]                           # count 8 > Kmax; count -1
    c["view"][2, 1] = 36                                          # a view index outside 0 .. P-1
    c["row"][3] = N_ROWS                                          # a store row outside 0 .. N-1
    c["view"][4] = 9                                              # 7 candidates in one view: 42 rows > V
    c["view"][0, 0], c["row"][0] = 35, N_ROWS - 1
    V = 41
    out = ViewOutputs(6, V, dims[1], dims[3])
    fill = out.numpy()
    want = ref.traj_views(c["img"], c["dep"], c["row"], c["count"], c["view"], c["loc"], c["tab"], V, dims[1], dims[3], fill=fill)
    assert want["status"].tolist() == [0, ref.ERR_COUNT, ref.ERR_VIEW, ref.ERR_ROW, ref.ERR_VIEWS, ref.ERR_COUNT]
    assert launch_views(on_device(c), c, V, out) == 0, _lib.lib().etp_last_error()
    for g in out.guards():
        g.check("malformed")
    got = out.numpy()
    same("malformed", got, want)
    for r in (1, 2, 3, 4, 5):
        assert got["rgb_fts"][r].tobytes() == fill["rgb_fts"][r].tobytes() and got["view_lens"][r] == -1


def test_traj_views_refusals_leave_everything_intact():
    c = view_case(3, DIMS[1])
    d = on_device(c)
    out = ViewOutputs(3, 45, 16, 8)
    fill = out.numpy()
    for override in (dict(Kmax=65), dict(P=65), dict(F_img=28), dict(F_img=18), dict(ld_dep=10), dict(N=0), dict(R=0), None):
        assert (launch_views(d, c, 45, out, **override) if override else launch_views(d, c, 0, out)) == -1, override   # None: V = 0
        assert b"etp_traj_views" in _lib.lib().etp_last_error()
    for g in out.guards():
        g.check("refusals")
    same("refusals", out.numpy(), fill)


# ---- etp_traj_pair_dists -----------------------------------------------------------------------------------------------------------
def dist_case(B, G, seed=0):
    rng = np.random.default_rng(seed + 17 * B + G)
    ns = (9, 40)
    tab = np.concatenate([rng.uniform(0.1, 40.0, n * n) for n in ns])           # asymmetric on purpose: [a][b] != [b][a]
    which = np.arange(B) % 2
    off = np.array([0, 81], dtype=np.int64)[which]
    n = np.array(ns, dtype=np.int32)[which]
    ln = rng.integers(1, G + 1, B).astype(np.int32)
    ln[0] = G
    idx = np.stack([rng.integers(0, n[b], G) for b in range(B)]).astype(np.int32)
    idx[:, 0] = -1                                                # [stop]
    for b in range(B):
        idx[b, ln[b]:] = -7                                      # padding: never looked at
    return {"tab": tab, "off": off, "n": n, "idx": idx, "len": ln}


class DistOutputs:
    def __init__(self, B, G):
        self.pair, self.mask, self.g_st = mr.guarded((B, G, G)), mr.guarded((B, G), torch.uint8), mr.guarded((B * 4,), torch.uint8)
        self.st = self.g_st.t.view(torch.int32)

    def guards(self):
        return [self.pair, self.mask, self.g_st]

    def numpy(self):
        return {"gmap_pair_dists": self.pair.t.cpu().numpy(), "gmap_masks": self.mask.t.cpu().numpy(), "status": self.st.cpu().numpy()}


def launch_dists(c, out, **override):
    d = {k: dev(c[k]) for k in ("tab", "off", "n", "idx", "len")}
    B, G = c["idx"].shape
    a = dict(dist_len=c["tab"].size, B=B, G=G)
    a.update(override)
    rc = _lib.lib().etp_traj_pair_dists(d["tab"].data_ptr(), a["dist_len"], d["off"].data_ptr(), d["n"].data_ptr(), d["idx"].data_ptr(),
                                        d["len"].data_ptr(), a["B"], a["G"], out.pair.t.data_ptr(), out.mask.t.data_ptr(), out.st.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("G", [1, 2, 9, 33, 70])
def test_traj_pair_dists_against_the_restatement(B, G):
    c = dist_case(B, G)
    want = ref.pair_dists(c["tab"], c["off"], c["n"], c["idx"], c["len"])
    assert not want["status"].any()
    if G >= 9:
        p = want["gmap_pair_dists"][0]
        assert (p == p.T).all() and (p[1:, 1:][~np.eye(G - 1, dtype=bool)] > 0).all() and not p[0].any() and not p.diagonal().any()
    out = DistOutputs(B, G)
    assert launch_dists(c, out) == 0, _lib.lib().etp_last_error()
    for g in out.guards():
        g.check(f"B{B} G{G}")
    got = out.numpy()
    same(f"B{B} G{G}", got, want)
    again = DistOutputs(B, G)
    assert launch_dists(c, again) == 0
    same(f"B{B} G{G} second run", again.numpy(), got)


def test_traj_pair_dists_flags_an_out_of_range_index_and_keeps_that_samples_fill():
    c = dist_case(3, 9, seed=5)
    c["len"][:] = [9, 9, 4]
    c["idx"][0, 1:] = np.arange(8)
    c["idx"][1, 1:9] = np.arange(8)
    c["idx"][1, 5] = 40                                           # sample 1 sits in the n = 40 block: 40 is one past its end
    c["idx"][0, 8] = 8                                            # sample 0, n = 9: the last valid index
    c["idx"][2, 3] = -1                                           # a negative index inside the length
    out = DistOutputs(3, 9)
    fill = out.numpy()
    want = ref.pair_dists(c["tab"], c["off"], c["n"], c["idx"], c["len"], fill=fill)
    assert want["status"].tolist() == [0, ref.ERR_INDEX, ref.ERR_INDEX]
    assert launch_dists(c, out) == 0, _lib.lib().etp_last_error()
    for g in out.guards():
        g.check("flagged")
    same("flagged", out.numpy(), want)
    c["off"][0], c["len"][2], c["idx"][2, 3] = 82 + 1600 - 80, 10, 0       # a block past the table's end; a length beyond G
    out = DistOutputs(3, 9)
    want = ref.pair_dists(c["tab"], c["off"], c["n"], c["idx"], c["len"], fill=out.numpy())
    assert want["status"].tolist() == [ref.ERR_SCAN, ref.ERR_INDEX, ref.ERR_LEN]
    assert launch_dists(c, out) == 0
    same("flagged scan / len", out.numpy(), want)
    fill = out.numpy()
    for override in (dict(B=0), dict(G=0), dict(dist_len=0)):
        assert launch_dists(c, out, **override) == -1
    same("refusals", out.numpy(), fill)


# ---- the native loaders on the recording -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def resident():
    c = ref.corpus()
    c["store"].to_device(DEV)
    c["graphs"].to_device(DEV)
    return c


@pytest.mark.parametrize("act", [False, True])
def test_sap_batches_reproduce_the_recorded_collate_output(resident, act):
    index = ref.make_index(act)
    samples = [tuple(x) for x in ref.js("samples")]
    sap = pdata.SapBatches(index, 4, np.random.default_rng(0), DEV)
    got = sap.batch(samples)
    sap.check()
    assert ref.differing(got, ref.expected("sap_all", visited_act=act)) == []
    again = sap.batch(samples)
    assert ref.differing(again, {k: (v.cpu().numpy() if k != "traj" else v) for k, v in got.items()}) == []
    if not act:
        two = sap.batch([samples[0], samples[5]])                 # other batch maxima: other padding
        sap.check()
        assert ref.differing(two, ref.expected("sap_two")) == []
    assert all(got[k].is_cuda for k in got if k != "traj")


def test_mlm_batches_reproduce_the_recorded_collate_output(resident):
    mlm = pdata.MlmBatches(ref.make_index(), 4, np.random.default_rng(0), DEV)
    got = mlm.batch(ref.js("mlm_items"), ref.mlm_uniforms())
    mlm.check()
    want = ref.expected("mlm_all")
    assert ref.differing(got, want) == []
    assert not got["txt_labels"].is_cuda and got["rgb_fts"].is_cuda


def test_iteration_draws_from_the_generator_and_check_reads_the_status(resident):
    index = ref.make_index()
    a = [b for b in pdata.SapBatches(index, 2, np.random.default_rng(7), DEV)]
    b = [b for b in pdata.SapBatches(index, 2, np.random.default_rng(7), DEV)]
    assert len(a) == 3 and [x["rgb_fts"].shape[0] for x in a] == [x["rgb_fts"].shape[0] for x in b]
    for x, y in zip(a, b):
        assert ref.differing(x, {k: (v.cpu().numpy() if k != "traj" else v) for k, v in y.items()}) == []
    sap = pdata.SapBatches(index, 2, np.random.default_rng(7), DEV)
    rec = dict(index.record(0, None))
    rec["rows"] = rec["rows"].copy()
    rec["rows"][1] = 18                                           # one past the store's last row: flagged on the device, never indexed
    sap.assemble([rec], [rec["txt"]], np.zeros(1, np.int64))
    with pytest.raises(_lib.EtpError, match="steps \\[1\\]"):
        sap.check()


def test_one_train_step_per_task_off_the_native_loaders():
    from oracle.make_golden_pretrain import make_case
    from etpnav_amd.planner import GlocalTextPathNavCMT
    from etpnav_amd.pretrain import PretrainDriver
    cfg, P, _ = make_case()
    c = ref.corpus()
    rng = np.random.default_rng(1)
    keys = c["keys"]
    with tempfile.TemporaryDirectory() as td:                      # the same corpus over a store of the model's widths
        write_flat_pack(os.path.join(td, "img.etpf"), ((k, rng.standard_normal((36, cfg.image_feat_size)).astype(np.float32)) for k in keys))
        write_flat_pack(os.path.join(td, "dep.etpf"), ((k, rng.standard_normal((36, cfg.depth_feat_size)).astype(np.float32)) for k in keys))
        store = FeatureStore(os.path.join(td, "img.etpf"), os.path.join(td, "dep.etpf")).to_device(DEV)
    graphs = pdata.NavGraphs.from_connectivity(ref.js("connectivity")).to_device(DEV)
    annos = [dict(a, instr_encoding=[101] + [1000 + t % 1000 for t in a["instr_encoding"][1:-1]] + [102]) for a in c["annos"]]
    index = pdata.R2RTextPathIndex([annos], store, c["cands"], graphs, cfg.image_feat_size, cfg.depth_feat_size, 16)
    gen = np.random.default_rng(3)
    sap = pdata.SapBatches(index, 3, gen, DEV)
    mlm = pdata.MlmBatches(index, 3, gen, DEV, vocab_range=(1000, 2000))
    model = GlocalTextPathNavCMT(cfg.to_dict(), dtype=torch.float32, device=DEV)
    model.load_state_dict(dict(P), strict=True)
    drv = PretrainDriver(model, {"sap": (sap, 1, None), "mlm": (mlm, 1, None)}, learning_rate=1e-4, warmup_steps=2, num_train_steps=10,
                         dropout=None)
    try:
        for name, src in (("sap", sap), ("mlm", mlm)):
            batch = next(iter(src))
            src.check()
            loss = float(drv.train_step(name, batch).item())
            assert np.isfinite(loss) and loss > 0, (name, loss)
    finally:
        drv.close()
