"""CPU-side checks of the pre-training data path's boundary (in the style of tests/test_pano_inputs_boundary_cpu.py): the two entry points of
csrc/traj_batch.hip are declared and exported, every refusal their header comment lists comes back as ETP_ERR_INVALID without a GPU
(nothing is launched: the operands are addresses that are never read), the build compiles the file under the row kernels' flags with
-ffp-contract=off, and the host layer raises ValueError before anything is launched: more than 64 candidates at a viewpoint, an unknown
key, a store that is not on the device, no GPU at all."""
import numpy as np
import pytest
import torch

from etpnav_amd import _lib, build
from etpnav_amd import pretrain_data as pdata
from tests import pretrain_data_ref as ref

P = 0x10000          # an aligned address; never dereferenced by a refused call
V_ARGS = ["img_store", "dep_store", "pano_row", "cand_count", "cand_view", "cand_loc", "view_loc_tab", "R", "V", "Kmax", "P", "F_img", "ld_img",
          "F_dep", "ld_dep", "N", "rgb_fts", "dep_fts", "loc_fts", "nav_types", "view_lens", "status"]
V_SCALARS = ("R", "V", "Kmax", "P", "F_img", "ld_img", "F_dep", "ld_dep", "N")
D_ARGS = ["dist_tab", "dist_len", "scan_off", "scan_n", "gmap_idx", "gmap_len", "B", "G", "gmap_pair_dists", "gmap_masks", "status"]
D_SCALARS = ("dist_len", "B", "G")


def views(**kw):
    a = {k: P for k in V_ARGS}
    a.update(R=3, V=38, Kmax=5, P=36, F_img=16, ld_img=24, F_dep=8, ld_dep=8, N=18)
    a.update(kw)
    return _lib.lib().etp_traj_views(*[a[k] for k in V_ARGS], None)


def dists(**kw):
    a = {k: P for k in D_ARGS}
    a.update(dist_len=162, B=2, G=9)
    a.update(kw)
    return _lib.lib().etp_traj_pair_dists(*[a[k] for k in D_ARGS], None)


def test_symbols_flags_and_citations():
    protos = _lib.parse_header()
    for name, args in (("etp_traj_views", V_ARGS), ("etp_traj_pair_dists", D_ARGS)):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
        assert len(protos[name][1]) == len(args) + 1
    hdr = open(_lib.HEADER).read()
    for sym, val in (("COUNT", ref.ERR_COUNT), ("VIEW", ref.ERR_VIEW), ("ROW", ref.ERR_ROW), ("VIEWS", ref.ERR_VIEWS), ("LEN", ref.ERR_LEN),
                     ("SCAN", ref.ERR_SCAN), ("INDEX", ref.ERR_INDEX)):
        assert f"#define ETP_TRAJ_ERR_{sym} {val}\n" in hdr
        assert getattr(pdata, f"TRAJ_ERR_{sym}") == val
    doc = hdr[hdr.index("A pre-training batch's device side"):hdr.index("int etp_traj_views")]
    assert "dataset.py:483-526" in doc and "tasks.py:331-343" in doc and "dataset.py:316-320" in doc and "tasks.py:350-355" in doc


V_REFUSALS = {"R 0": dict(R=0), "V 0": dict(V=0), "N 0": dict(N=0), "N -1": dict(N=-1), "Kmax 0": dict(Kmax=0), "Kmax 65": dict(Kmax=65),
              "P 0": dict(P=0), "P 65": dict(P=65), "F_img 0": dict(F_img=0), "F_img 18": dict(F_img=18), "F_img > ld_img": dict(F_img=28),
              "ld_img 26": dict(ld_img=26), "F_dep 0": dict(F_dep=0), "F_dep 6": dict(F_dep=6), "F_dep > ld_dep": dict(F_dep=12),
              "ld_dep 10": dict(ld_dep=10), "dep_store without dep_fts": dict(dep_fts=None), "dep_fts without dep_store": dict(dep_store=None),
              "misaligned img_store": dict(img_store=P + 8), "misaligned dep_store": dict(dep_store=P + 4),
              "misaligned rgb_fts": dict(rgb_fts=P + 8), "misaligned dep_fts": dict(dep_fts=P + 4),
              "misaligned nav_types": dict(nav_types=P + 4), "misaligned view_lens": dict(view_lens=P + 4),
              "misaligned pano_row": dict(pano_row=P + 2), "misaligned cand_count": dict(cand_count=P + 1),
              "misaligned cand_view": dict(cand_view=P + 2), "misaligned cand_loc": dict(cand_loc=P + 2),
              "misaligned view_loc_tab": dict(view_loc_tab=P + 2), "misaligned loc_fts": dict(loc_fts=P + 1),
              "misaligned status": dict(status=P + 2)}
V_REFUSALS.update({f"NULL {k}": {k: None} for k in V_ARGS if k not in V_SCALARS + ("dep_store", "dep_fts")})
D_REFUSALS = {"B 0": dict(B=0), "G 0": dict(G=0), "dist_len 0": dict(dist_len=0), "misaligned dist_tab": dict(dist_tab=P + 4),
              "misaligned scan_off": dict(scan_off=P + 4), "misaligned scan_n": dict(scan_n=P + 2), "misaligned gmap_idx": dict(gmap_idx=P + 1),
              "misaligned gmap_len": dict(gmap_len=P + 2), "misaligned gmap_pair_dists": dict(gmap_pair_dists=P + 2),
              "misaligned status": dict(status=P + 2)}
D_REFUSALS.update({f"NULL {k}": {k: None} for k in D_ARGS if k not in D_SCALARS})


@pytest.mark.parametrize("name", list(V_REFUSALS))
def test_traj_views_refusals_come_back_before_anything_is_launched(name):
    assert views(**V_REFUSALS[name]) == -1, name
    assert b"etp_traj_views" in _lib.lib().etp_last_error()


@pytest.mark.parametrize("name", list(D_REFUSALS))
def test_traj_pair_dists_refusals_come_back_before_anything_is_launched(name):
    assert dists(**D_REFUSALS[name]) == -1, name
    assert b"etp_traj_pair_dists" in _lib.lib().etp_last_error()


def test_build_lists_the_file_with_the_row_kernel_flags():
    assert "traj_batch.hip" in build.SOURCES and "traj_batch.hip" in build.NO_PACKED_FP32
    flags = build.PER_SOURCE_FLAGS["traj_batch.hip"]
    assert "-fno-slp-vectorize" in flags and "-ffp-contract=off" in flags
    src = open(build.CSRC + "/traj_batch.hip").read()
    assert "atomic" not in src.replace("no atomics", "") and "__shared__" not in src
    for fn in ("sinf", "cosf", "expf", "__sinf", "__cosf"):
        assert fn + "(" not in src, fn


def test_too_many_candidates_and_unknown_keys_raise_before_any_launch():
    c = ref.corpus()
    cands = dict(c["cands"])
    key = next(iter(cands))
    cands[key] = {f"x{i}": [i % 36, 1.0, 0.0, 0.0] for i in range(65)}
    with pytest.raises(ValueError, match="65 candidates"):
        pdata.R2RTextPathIndex([c["annos"]], c["store"], cands, c["graphs"], 16, 8, 16)
    cands[key] = {"x": [36, 1.0, 0.0, 0.0]}
    with pytest.raises(ValueError, match="view index"):
        pdata.R2RTextPathIndex([c["annos"]], c["store"], cands, c["graphs"], 16, 8, 16)
    index = ref.make_index()
    index.data.append(dict(c["annos"][0], path=["nowhere"]))
    with pytest.raises(ValueError, match="unknown key"):
        index.record(len(index.data) - 1, None)
    index.data[-1] = dict(c["annos"][0], scan="scanZ")
    with pytest.raises(ValueError, match="unknown key"):
        index.record(len(index.data) - 1, None)
    with pytest.raises(ValueError, match="end index"):
        index.record(0, 9)


def test_loaders_fail_loudly_without_a_device_resident_store():
    index = ref.make_index()
    gen = np.random.default_rng(0)
    for cls in (pdata.SapBatches, pdata.MlmBatches):
        with pytest.raises(ValueError, match="no CPU fallback"):
            cls(index, 2, gen, "cpu")
        if not torch.cuda.is_available():
            assert index.store._dev is None
            with pytest.raises(ValueError, match="not on the device"):
                cls(index, 2, gen, "cuda:0")
