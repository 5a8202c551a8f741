"""tests/pretrain_data_ref.py and the host layer of etpnav_amd/pretrain_data.py pinned to the recording of the REAL reference classes
(tests/golden/pretrain_batch_small.npz, written by tools/make_golden_pretrain_batch.py), without a GPU:

  * the restatement (get_input + collate) and the host layer (R2RTextPathIndex records -> staging arrays -> the kernels' restatement)
    give every recorded tensor of sap_collate / mlm_collate bit for bit and every list equal, act_visited_node on and off;
  * NavGraphs gives load_nav_graphs' recorded distances bit for bit and its hop counts, and networkx's own where it imports;
  * mask_tokens gives the recorded random_word output, and its branch frequencies over 200 000 uniforms lie within 4 sigma of
    0.15 * (0.8, 0.1, 0.1);
  * nine planted mutations of the restatement are rejected by the same comparison.
"""
import json

import numpy as np
import pytest

from etpnav_amd import pretrain_data as pdata
from tests import pretrain_data_ref as ref

SAMPLES = [tuple(x) for x in ref.js("samples")]


@pytest.mark.parametrize("prefix,pick", [("sap_all", None), ("sap_two", (0, 5))])
@pytest.mark.parametrize("act", [False, True])
def test_restatement_and_host_layer_reproduce_the_recorded_sap_batches(prefix, pick, act):
    samples = SAMPLES if pick is None else [SAMPLES[k] for k in pick]
    want = ref.expected(prefix, visited_act=act and prefix == "sap_all")
    if act and prefix != "sap_all":
        want.pop("gmap_visited_masks")
    assert ref.differing(ref.sap_batch(samples, act), want) == []
    index = ref.make_index(act)
    recs = [index.record(i, e) for i, e in samples]
    got = ref.host_layer_batch(index, recs, [r["txt"] for r in recs], [r["global_act_label"] for r in recs])
    assert ref.differing(got, want) == []
    f = ref.fixture()
    assert [r["local_act_label"] for r in recs] == f[f"{prefix}_local_act_labels"].tolist()


def test_recording_covers_the_cases_the_kernels_can_get_wrong():
    w = ref.expected("sap_all")
    assert w["view_lens"].max() > 36 and w["rgb_fts"].shape[2] == 16 < ref.fixture()["store_img"].shape[2]
    assert 1 in w["traj"]["traj_step_lens"] and 21 in w["traj"]["traj_step_lens"]
    assert w["labels"][1] == 0 and (w["labels"] > 0).any()
    assert min(len(c) for ep in w["traj"]["traj_cand_vpids"] for c in ep) == 1


def test_restatement_and_host_layer_reproduce_the_recorded_mlm_batch():
    want = ref.expected("mlm_all")
    items, uni = ref.js("mlm_items"), ref.mlm_uniforms()
    assert ref.differing(ref.mlm_batch(items, uni), want) == []
    index = ref.make_index()
    recs = [index.record(i, None) for i in items]
    masked = [pdata.mask_tokens(r["txt"], u, u2=u2) for r, (u, u2) in zip(recs, uni)]
    got = ref.host_layer_batch(index, recs, [m[0] for m in masked], [0] * len(recs), [m[1] for m in masked])
    assert ref.differing(got, want) == []
    lab = want["txt_labels"]
    assert (lab[2] != -1).sum() == 1 and lab[2, 0] != -1 and want["txt_ids"][2, 0] == pdata.MASK_TOKEN_ID      # "at least mask 1"
    assert want["txt_ids"][1, 0] == pdata.MASK_TOKEN_ID and pdata.VOCAB_RANGE[0] <= want["txt_ids"][1, 1] < pdata.VOCAB_RANGE[1]
    assert want["txt_ids"][1, 2] == lab[1, 2] and want["txt_ids"].shape[1] == 16                               # keep; max_txt_len


def test_nav_graphs_reproduce_load_nav_graphs():
    f, g = ref.fixture(), ref.corpus()["graphs"]
    for scan in ref.js("scans"):
        s = g.scans[scan]
        assert s["vps"] == ref.js(f"nav_{scan}_nodes")
        assert s["dist"].tobytes() == f[f"nav_{scan}_dist"].tobytes()
        assert (s["hops"] == f[f"nav_{scan}_hops"]).all() and s["pos"].tobytes() == f[f"nav_{scan}_pos"].tobytes()
    assert g.dist_len == sum(len(s["vps"]) ** 2 for s in g.scans.values()) and list(g.offset.values()) == [0, 81]


def test_nav_graphs_against_networkx():
    nx = pytest.importorskip("networkx")
    conn, g = ref.js("connectivity"), ref.corpus()["graphs"]
    for scan, data in conn.items():
        G = nx.Graph()
        for i, item in enumerate(data):
            for j, c in enumerate(item["unobstructed"]):
                if c:
                    a, b = item["pose"], data[j]["pose"]
                    G.add_edge(item["image_id"], data[j]["image_id"],
                               weight=((a[3] - b[3]) ** 2 + (a[7] - b[7]) ** 2 + (a[11] - b[11]) ** 2) ** 0.5)
        d, p = dict(nx.all_pairs_dijkstra_path_length(G)), dict(nx.all_pairs_dijkstra_path(G))
        s = g.scans[scan]
        assert s["vps"] == list(G.nodes)
        for x in s["vps"]:
            for y in s["vps"]:
                assert s["dist"][s["index"][x], s["index"][y]] == d[x][y] and s["hops"][s["index"][x], s["index"][y]] == len(p[x][y]) - 1


def test_mask_tokens_branch_frequencies():
    n = 200000
    rng = np.random.default_rng(0)
    tok = np.full(n, 5000, dtype=np.int64)
    ids, labels = pdata.mask_tokens(tok, rng.random(n), u2=rng.random(n))
    drawn = labels != -1
    counts = [(drawn & (ids == pdata.MASK_TOKEN_ID)).sum(), (drawn & (ids != pdata.MASK_TOKEN_ID) & (ids != 5000)).sum()]
    counts.append(drawn.sum() - sum(counts))                     # kept (a random word equal to the token counts here: 1 in 27615)
    for c, p in zip(counts, (0.12, 0.015, 0.015)):
        assert abs(c - n * p) <= 4 * np.sqrt(n * p * (1 - p)) + (n * 0.015 / 27615 + 1), (c, p)
    word = ids[drawn & (ids != pdata.MASK_TOKEN_ID) & (ids != 5000)]
    assert word.min() >= pdata.VOCAB_RANGE[0] and word.max() < pdata.VOCAB_RANGE[1]
    with pytest.raises(ValueError):
        pdata.mask_tokens([1, 2], [0.5])


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_planted_mutations_are_rejected(mutation):
    want = ref.expected("sap_all")
    assert ref.differing(ref.sap_batch(SAMPLES), want) == []
    try:
        bad = ref.sap_batch(SAMPLES, mutate=mutation)
    except ValueError:                                           # the slice dropped: the steps no longer stack
        assert mutation == "slice_dropped"
        return
    assert ref.differing(bad, want) != [], mutation


def test_kernel_restatement_flags_each_malformed_condition_for_that_step_only():
    c = ref.corpus()
    tab = pdata.angle_fts(*pdata.view_rel_angles(12).T)
    row, cnt = np.array([0, 1, 2, 99, 4], np.int32), np.array([1, 9, 1, 1, 2], np.int32)
    view = np.zeros((5, 2), np.int32)
    view[2, 0] = 36
    view[4] = [3, 5]
    out = ref.traj_views(c["img"], c["dep"], row, cnt, view, np.zeros((5, 2, 4), np.float32), tab, 37, 16, 8)
    assert out["status"].tolist() == [0, ref.ERR_COUNT, ref.ERR_VIEW, ref.ERR_ROW, 0] and out["view_lens"].tolist() == [36, 0, 0, 0, 36]
    out = ref.traj_views(c["img"], c["dep"], row, cnt, view, np.zeros((5, 2, 4), np.float32), tab, 35, 16, 8)
    assert out["status"].tolist() == [ref.ERR_VIEWS, ref.ERR_COUNT, ref.ERR_VIEW | ref.ERR_VIEWS, ref.ERR_ROW | ref.ERR_VIEWS, ref.ERR_VIEWS]
    assert (pdata.TRAJ_ERR_COUNT, pdata.TRAJ_ERR_VIEW, pdata.TRAJ_ERR_ROW, pdata.TRAJ_ERR_VIEWS) == (1, 2, 4, 8)
    json.dumps(ref.MUTATIONS)
