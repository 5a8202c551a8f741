"""CPU-side checks of the trajectory node features' boundary (in the style of tests/test_pretrain_data_boundary_cpu.py): the two entry
points are declared and exported with their two new status codes, every refusal their header comment lists comes back as ETP_ERR_INVALID
without a GPU (nothing is launched: the operands are addresses that are never read), the host layer fails loudly without a GPU, and the
loaders' TrajBatch is the old batch dict, key for key."""
import numpy as np
import pytest
import torch

from etpnav_amd import _lib, build
from etpnav_amd import graph_inputs as gi
from etpnav_amd import pretrain_data as pdata
from tests import traj_nodes_ref as tr

P = 0x10000          # an aligned address; never dereferenced by a refused call
TABLES = ["step_off", "step_vp", "view_lens", "cand_count", "cand_vp", "gmap_id", "gmap_len"]
SCALARS = ["B", "R", "V", "Kmax", "G", "H"]
ENTRY = {"etp_traj_nodes_fwd": ["pano"] + TABLES + SCALARS + ["gmap_img_fts", "status"],
         "etp_traj_nodes_bwd": ["d_gmap_img_fts"] + TABLES + SCALARS + ["d_pano", "status"]}


def call(name, **kw):
    a = {k: P for k in ENTRY[name]}
    a.update(B=2, R=5, V=7, Kmax=4, G=6, H=768)
    a.update(kw)
    return getattr(_lib.lib(), name)(*[a[k] for k in ENTRY[name]], None)


def test_symbols_codes_and_citations():
    protos = _lib.parse_header()
    for name, args in ENTRY.items():
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
        assert len(protos[name][1]) == len(args) + 1
    hdr = open(_lib.HEADER).read()
    for sym, val in (("STEPS", tr.ERR_STEPS), ("NODE", tr.ERR_NODE), ("COUNT", tr.ERR_COUNT), ("VIEWS", tr.ERR_VIEWS), ("LEN", tr.ERR_LEN)):
        assert f"#define ETP_TRAJ_ERR_{sym} {val}\n" in hdr
    assert (gi.TRAJ_ERR_COUNT_OR_LEN, gi.TRAJ_ERR_VIEWS, gi.TRAJ_ERR_STEPS, gi.TRAJ_ERR_NODE) == (tr.ERR_COUNT, tr.ERR_VIEWS, tr.ERR_STEPS, tr.ERR_NODE)
    doc = hdr[hdr.index("Trajectory node features straight from"):hdr.index("int etp_traj_nodes_fwd")]
    assert "vilmodel.py:585-619" in doc and "etp_gather_sum" in doc and "ascending node index" in doc and "LAST" in doc
    assert len({tr.ERR_COUNT, tr.ERR_VIEWS, tr.ERR_STEPS, tr.ERR_NODE}) == 4


def _refusals(name):
    rows, out = ENTRY[name][0], ENTRY[name][-2]
    r = {"H 0": dict(H=0), "H 128": dict(H=128), "H 1024": dict(H=1024), "H 640": dict(H=640), "B 0": dict(B=0), "R 0": dict(R=0),
         "V 0": dict(V=0), "G 0": dict(G=0), "B -1": dict(B=-1), "Kmax 0": dict(Kmax=0), "Kmax 65": dict(Kmax=65),
         "B*G beyond the grid": dict(B=1 << 20, G=1 << 10), "R*V beyond the grid": dict(R=1 << 20, V=1 << 10),
         f"misaligned {rows}": {rows: P + 8}, f"misaligned {out}": {out: P + 4}, "misaligned view_lens": dict(view_lens=P + 4),
         "misaligned status": dict(status=P + 2)}
    r.update({f"misaligned {k}": {k: P + 2} for k in TABLES if k != "view_lens"})
    r.update({f"NULL {k}": {k: None} for k in ENTRY[name] if k not in SCALARS})
    return r


@pytest.mark.parametrize("entry,name", [(e, n) for e in ENTRY for n in _refusals(e)])
def test_refusals_come_back_before_anything_is_launched(entry, name):
    assert call(entry, **_refusals(entry)[name]) == -1, name
    assert entry.encode() in _lib.lib().etp_last_error()


def test_kernels_keep_the_files_idiom():
    """no LDS, no atomics (tests/test_pretrain_data_boundary_cpu.py checks the same of the whole file), rows through row.h, the fused
    multiply-add spelled out under -ffp-contract=off"""
    src = open(build.CSRC + "/traj_batch.hip").read()
    assert '#include "row.h"' in src and "ETP_DISPATCH_H(H" in src and "fmaf(" in src
    assert "-ffp-contract=off" in build.PER_SOURCE_FLAGS["traj_batch.hip"]
    assert "row.h" in build.HEADERS


def test_the_table_route_fails_loudly_without_a_gpu():
    traj = tr.crafted(5)
    td = gi.traj_descriptors(traj, 9, "cpu")
    with pytest.raises(_lib.EtpError, match="no CPU fallback"):
        gi.aggregate_gmap_features(torch.zeros(9, 5, 256), traj["traj_vp_lens"], None, None, None, 9, traj_dev=td)
    with pytest.raises(_lib.EtpError, match="no CPU fallback"):
        gi.aggregate_gmap_features(torch.zeros(9, 5, 256), traj["traj_vp_lens"], traj["traj_vpids"], traj["traj_cand_vpids"],
                                   traj["gmap_vpids"], 9)


def test_status_message_names_rows_and_steps():
    st = np.zeros(2 * 6 + 5, np.int32)
    assert gi.traj_status_message(st, 12, 6) is None
    st[7], st[12 + 3] = tr.ERR_NODE, tr.ERR_STEPS
    msg = gi.traj_status_message(st, 12, 6)
    assert "(sample 1, node 1): 32" in msg and "step 3: 16" in msg


def test_traj_batch_is_the_old_dict_key_for_key():
    old = {"rgb_fts": 1, "traj": {"traj_vpids": [["a"]]}, "labels": 3}
    tb = pdata.TrajBatch(old)
    assert isinstance(tb, dict) and tb == old and list(tb) == list(old) and "traj_dev" not in tb
    assert tb.traj_dev is None
    tb.traj_dev = {"Kmax": 1}
    assert tb == old and list(tb.keys()) == list(old.keys()) and dict(tb) == old
    assert getattr(old, "traj_dev", None) is None             # what the step asks of a plain dict
