"""CPU-side checks of the device-resident map's boundary (in the style of tests/test_decide_boundary_cpu.py): the four entry points of
csrc/gmap_update.hip are declared and exported, every refusal their header comment lists comes back as ETP_ERR_INVALID without a GPU
(nothing is launched: the operands are addresses that are never read), the host mirror fails loudly without a GPU and keeps the
reference's names, and the build compiles the file under the row kernels' flags with contraction off."""
import numpy as np
import pytest
import torch

from etpnav_amd import _lib, build, decide, graph_inputs
from tests import gmap_update_ref as gr

P = 0x10000          # an aligned address; never dereferenced by a refused call
UPDATE_ARGS = ["state", "S", "slot", "prev_node", "step_id", "cur_pos", "cur_heading", "cand_pos", "n_cand", "cur_row", "cand_row", "del_ghost",
               "noise", "loc_noise", "merge_ghost", "ghost_aug", "B", "Kmax", "node_pos", "node_step", "n_nodes", "adj", "ghost_pos", "n_ghost",
               "front_ptr", "front_idx", "cur_node", "cur_pos_out", "cur_heading_out", "record"]
CSR_ARGS = ["state", "S", "slot", "B", "G", "R", "ptr_f", "idx_f", "w_f", "ptr_b", "idx_b", "w_b", "status"]


def update(**kw):
    a = {k: P for k in UPDATE_ARGS}
    a.update(S=2, noise=None, loc_noise=0.5, merge_ghost=1, ghost_aug=0.0, B=2, Kmax=16)
    a.update(kw)
    return _lib.lib().etp_gmap_update(*[a[k] for k in UPDATE_ARGS], None)


def csr(**kw):
    a = {k: P for k in CSR_ARGS}
    a.update(S=2, B=2, G=8, R=10)
    a.update(kw)
    return _lib.lib().etp_gmap_embed_csr(*[a[k] for k in CSR_ARGS], None)


def test_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    for name, nargs in (("etp_gmap_slot_bytes", 0), ("etp_gmap_reset", 5), ("etp_gmap_update", 31), ("etp_gmap_embed_csr", 14)):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name) and len(protos[name][1]) == nargs, name
    nbytes = _lib.lib().etp_gmap_slot_bytes()
    # doubles: 64 node positions, 192 sums and means; fp32 adj 64 x 64; int32: steps, rows, ids, 193 pointers, 2 x FMAX entries, 3 counts
    assert nbytes == 8 * 3 * (64 + 2 * 192) + 4 * 64 * 64 + 4 * (64 + 64 + 192 + 193 + 2 * graph_inputs.GMAP_FMAX + 3) and nbytes % 16 == 0
    assert (graph_inputs.GMAP_FMAX, graph_inputs.GMAP_HDR, graph_inputs.GMAP_KMAX) == (gr.FMAX, gr.HDR, gr.KMAX) == (512, 8, 16)
    assert (graph_inputs.GMAP_ERR_CAPACITY, graph_inputs.GMAP_ERR_INPUT, graph_inputs.GMAP_ERR_ROW) == (gr.ERR_CAPACITY, gr.ERR_INPUT, gr.ERR_ROW) == (1, 2, 4)
    assert (graph_inputs.GMAP_EDGE, graph_inputs.GMAP_NEW, graph_inputs.GMAP_MERGED) == (gr.EDGE, gr.NEW, gr.MERGED) == (1, 2, 3)


UPDATE_REFUSALS = {
    "B 0": dict(B=0), "B -1": dict(B=-1), "S 0": dict(S=0), "Kmax 17": dict(Kmax=17), "Kmax 0": dict(Kmax=0),
    "misaligned state": dict(state=P + 8), "misaligned cur_pos": dict(cur_pos=P + 4), "misaligned cand_pos": dict(cand_pos=P + 4),
    "misaligned noise": dict(noise=P + 4), "misaligned slot": dict(slot=P + 2), "misaligned record": dict(record=P + 2),
    "misaligned adj": dict(adj=P + 1), "misaligned front_idx": dict(front_idx=P + 2), "misaligned cur_heading": dict(cur_heading=P + 2),
    **{f"NULL {k}": {k: None} for k in UPDATE_ARGS if k not in ("S", "noise", "loc_noise", "merge_ghost", "ghost_aug", "B", "Kmax")},
}
CSR_REFUSALS = {"B 0": dict(B=0), "S 0": dict(S=0), "R 0": dict(R=0), "G 0": dict(G=0), "G 258": dict(G=258), "misaligned state": dict(state=P + 4),
                "misaligned ptr_b": dict(ptr_b=P + 2), "misaligned w_f": dict(w_f=P + 1),
                **{f"NULL {k}": {k: None} for k in CSR_ARGS if k not in ("S", "B", "G", "R")}}


@pytest.mark.parametrize("name", list(UPDATE_REFUSALS))
def test_update_refusals_come_back_before_anything_is_launched(name):
    assert update(**UPDATE_REFUSALS[name]) == -1, name
    assert b"etp_gmap_update" in _lib.lib().etp_last_error()


@pytest.mark.parametrize("name", list(CSR_REFUSALS))
def test_embed_csr_refusals_come_back_before_anything_is_launched(name):
    assert csr(**CSR_REFUSALS[name]) == -1, name
    assert b"etp_gmap_embed_csr" in _lib.lib().etp_last_error()


def test_reset_refusals():
    L = _lib.lib()
    for args in ((None, 2, P, 1), (P, 2, None, 1), (P, 0, P, 1), (P, 2, P, 0), (P + 8, 2, P, 1), (P, 2, P + 2, 1)):
        assert L.etp_gmap_reset(*args, None) == -1, args
        assert b"etp_gmap_reset" in L.etp_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_compute_fails_loudly_without_gpu():
    maps = graph_inputs.DeviceGraphMaps(2, "cpu", False, 0.5, True, 0.0)
    cur_vp, cand_vp, cand_pos = maps.identify_node(np.zeros((2, 3)), [0.0, 1.0], [[0.5], [1.0, 2.0]], [[1.0], [1.5, 2.0]])
    with pytest.raises(_lib.EtpError):
        maps.update([None, None], 1, cur_vp, np.zeros((2, 3)), [0.0, 1.0], cand_pos, [0, 2], [[1], [3, 4]])
    for call in (maps.compact, maps.nav_inputs, lambda: maps.embed_csr(4, 8), lambda: maps.img_fts(torch.zeros(8, 256), 4)):
        with pytest.raises(_lib.EtpError):
            call()


def test_host_mirror_bookkeeping_names_and_identify_node():
    maps = graph_inputs.DeviceGraphMaps(4, "cpu", True, 0.5, True, 0.3)
    assert maps.active == [0, 1, 2, 3] and len(maps.gmaps) == 4
    maps.pause(1)
    assert maps.active == [0, 2, 3] and maps.gmaps[1] is maps.views[2]
    # identify_node: GraphMapLite's arithmetic, bit for bit, for the whole batch
    pos, heading = np.array([[1.0, 0.2, -3.0], [0.5, 0.0, 2.0], [0.0, 0.0, 0.0]]), [0.3, 5.9, 1.0]
    ang, dis = [[0.1, 2.0, 6.0], [], [3.0]], [[1.0, 2.2, 0.7], [], [1.5]]
    cur_vp, cand_vp, cand_pos = maps.identify_node(pos, heading, ang, dis)
    lite = graph_inputs.GraphMapLite(False, 0.5, True, 0)
    for i in range(3):
        want = lite.identify_node(pos[i], heading[i], ang[i], dis[i])
        assert cur_vp[i] == want[0] == "0" and cand_vp[i] == want[1] and len(cand_pos[i]) == len(want[2])
        assert all(np.array_equal(a, b) for a, b in zip(cand_pos[i], want[2]))
    # the views follow a record without any arithmetic on distances; names are the reference's
    rec = np.full((3, 24), -1, np.int32)
    rec[:, :8] = [[1, 2, 0, 0, 2, 3, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 1, 1, 0, 0]]
    rec[0, 8:11] = [gr.code(gr.NEW, 0), gr.code(gr.NEW, 1), gr.code(gr.MERGED, 0)]
    rec[2, 8] = gr.code(gr.NEW, 0)
    cq = np.zeros((3, 16, 3))
    for i in range(3):
        for k, p in enumerate(cand_pos[i]):
            cq[i, k] = p
    real = [[("r", i, k) for k in range(len(c))] for i, c in enumerate(cand_pos)]
    noise = np.full((3, 192, 3), 5.0)
    maps._mirror(rec, maps.gmaps, cur_vp, pos, 1, cq, real, noise)
    v = maps.gmaps[0]
    assert list(v.node_pos) == ["0"] and v.node_stepId == {"0": 1} and list(v.ghost_pos) == ["g0", "g1"] and v.ghost_cnt == 2
    assert v.ghost_fronts == {"g0": ["0", "0"], "g1": ["0"]} and v.ghost_real_pos == {"g0": [("r", 0, 0), ("r", 0, 2)], "g1": [("r", 0, 1)]}
    assert np.array_equal(v.ghost_mean_pos["g0"], (cq[0, 0] + cq[0, 2]) / 2.0)
    assert np.array_equal(v.ghost_aug_pos["g1"], cq[0, 1] + [0.3, 0.0, 0.3])          # 5 sigma clipped to ghost_aug
    assert maps.gmaps[1].ghost_pos == {} and list(maps.gmaps[2].ghost_pos) == ["g0"]
    v.delete_ghost("g0")
    assert v.pending_delete == 0 and list(v.ghost_pos) == ["g1"] and "g0" not in v.ghost_real_pos and "g0" not in v.ghost_aug_pos
    with pytest.raises(ValueError):
        v.delete_ghost("g1")
    # env_actions_from_record reads a view as it reads a GraphMapLite
    drec = np.array([[2, 2, 0, 0, 0, 0, 0, 0] + [-1] * 64], dtype=np.int32)
    act = decide.env_actions_from_record(drec, [v], ["0"], "control", True)[0]["action"]
    assert act["ghost_vp"] == "g1" and act["front_vp"] == "0" and np.array_equal(act["ghost_pos"], v.ghost_aug_pos["g1"])
    maps.reset()
    assert maps.active == [0, 1, 2, 3] and all(not x.node_pos for x in maps.views)


def test_update_refuses_on_the_host_what_the_kernel_would_flag():
    """before any launch (so also without a GPU): nothing has changed when the ValueError arrives"""
    maps = graph_inputs.DeviceGraphMaps(2, "cpu", False, 0.5, True, 0.0)
    pos, far = np.zeros((2, 3)), [[np.array([9.0, 0, 0])], []]
    args = lambda **kw: dict(dict(prev_vp=[None, None], step_ids=1, cur_vp=["0", "0"], cur_pos=pos, cur_heading=[0.0, 0.0], cand_pos=far,
                                  cur_rows=[0, 2], cand_rows=[[1], []]), **kw)
    for bad in (dict(prev_vp=["0", None]), dict(prev_vp=[None, "-1"]), dict(prev_vp=[None, "g0"]), dict(cur_rows=[0, -2]), dict(cand_rows=[[-1], []]),
                dict(cur_vp=["1", "0"]), dict(cand_pos=[[np.zeros(3)] * 17, []], cand_rows=[list(range(1, 18)), []])):
        with pytest.raises(ValueError):
            maps.update(**args(**bad))
    v = maps.gmaps[0]                                         # a full map: 64 nodes / 192 ghosts / 512 absorbed candidates
    v.node_pos = {str(i): np.zeros(3) for i in range(64)}
    with pytest.raises(ValueError, match="full"):
        maps.update(**args(cur_vp=["64", "0"]))
    v.node_pos = {}
    v.ghost_pos = {f"g{i}": [np.zeros(3)] for i in range(192)}
    v.ghost_fronts = {f"g{i}": ["0"] for i in range(192)}
    with pytest.raises(ValueError, match="full"):
        maps.update(**args())
    v.ghost_pos, v.ghost_fronts = {"g0": [np.zeros(3)] * 512}, {"g0": ["0"] * 512}
    with pytest.raises(ValueError, match="full"):
        maps.update(**args())
    v.ghost_pos, v.ghost_fronts = {}, {}
    if not torch.cuda.is_available():
        with pytest.raises(_lib.EtpError):                    # valid input gets as far as the missing GPU
            maps.update(**args())
    assert maps.gmaps[0].max_row == -1 and maps.gmaps[0].pending_delete == -1


def test_build_lists_the_file_with_the_row_kernel_flags_and_contraction_off():
    assert "gmap_update.hip" in build.SOURCES and "gmap_update.hip" in build.NO_PACKED_FP32
    assert "-ffp-contract=off" in build.PER_SOURCE_FLAGS["gmap_update.hip"] and "-fno-slp-vectorize" in build.PER_SOURCE_FLAGS["gmap_update.hip"]
    assert "-ffp-contract=off" not in build.PER_SOURCE_FLAGS["decide.hip"]
    src = open(build.CSRC + "/gmap_update.hip").read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.replace("no atomics", "")
