"""CPU-side checks of the embedding store's boundary (in the style of tests/test_gmap_update_boundary_cpu.py): the two entry points of
csrc/pano_store.hip are declared and exported, every refusal their header comment lists comes back as ETP_ERR_INVALID without a GPU
(nothing is launched: the operands are addresses that are never read), graph_inputs.EmbedStore refuses bad arguments and allocates
rows on the host, fails loudly where a launch is needed, and the build compiles the file under the row kernels' flags."""
import numpy as np
import pytest
import torch

from etpnav_amd import _lib, build, graph_inputs
from etpnav_amd.graph_inputs import EmbedStore
from tests import pano_store_ref as pr

P = 0x10000          # an aligned address; never dereferenced by a refused call
FWD_ARGS = ["pano_embeds", "pano_masks", "nav_types", "row_base", "n_cand", "B", "V", "H", "store", "R", "status"]
BWD_ARGS = ["d_store", "pano_masks", "nav_types", "row_base", "n_cand", "B", "V", "H", "R", "d_pano_embeds", "accumulate"]
SCALARS = ("B", "V", "H", "R", "accumulate")


def call(name, args, **kw):
    a = {k: P for k in args}
    a.update(B=2, V=6, H=768, R=10, accumulate=0)
    a.update(kw)
    return getattr(_lib.lib(), name)(*[a[k] for k in args], None)


def test_symbols_flags_and_limits():
    protos = _lib.parse_header()
    for name, nargs in (("etp_pano_store_fwd", 12), ("etp_pano_store_bwd", 12)):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name) and len(protos[name][1]) == nargs, name
    hdr = open(_lib.HEADER).read()
    for sym, val in (("EMPTY", pr.ERR_EMPTY), ("MASKED", pr.ERR_MASKED), ("COUNT", pr.ERR_COUNT), ("ROW", pr.ERR_ROW)):
        assert f"#define ETP_PSTORE_ERR_{sym} {val}\n" in hdr
        assert getattr(graph_inputs, f"PSTORE_ERR_{sym}") == val
    assert (graph_inputs.PSTORE_VMAX, graph_inputs.GMAP_KMAX) == (pr.VMAX, pr.KMAX) == (64, 16)
    # each declaration cites what it replaces
    doc = hdr[hdr.index("The embedding store's rows"):hdr.index("int etp_pano_store_fwd")]
    assert "ss_trainer_ETP.py:838-839, 864-869" in doc and "graph_utils.py:206,224,233" in doc


REFUSALS = {"H 128": dict(H=128), "H 1024": dict(H=1024), "H 0": dict(H=0), "V 0": dict(V=0), "V 65": dict(V=65), "B 0": dict(B=0),
            "B -1": dict(B=-1), "R 0": dict(R=0)}
FWD_REFUSALS = dict(REFUSALS, **{"misaligned pano_embeds": dict(pano_embeds=P + 8), "misaligned store": dict(store=P + 4),
                                  "misaligned nav_types": dict(nav_types=P + 4), "misaligned row_base": dict(row_base=P + 2),
                                  "misaligned n_cand": dict(n_cand=P + 1), "misaligned status": dict(status=P + 2)},
                    **{f"NULL {k}": {k: None} for k in FWD_ARGS if k not in SCALARS})
BWD_REFUSALS = dict(REFUSALS, **{"misaligned d_store": dict(d_store=P + 8), "misaligned d_pano_embeds": dict(d_pano_embeds=P + 4),
                                  "misaligned nav_types": dict(nav_types=P + 4), "accumulate 2": dict(accumulate=2),
                                  "accumulate -1": dict(accumulate=-1)},
                    **{f"NULL {k}": {k: None} for k in BWD_ARGS if k not in SCALARS})


@pytest.mark.parametrize("name", list(FWD_REFUSALS))
def test_fwd_refusals_come_back_before_anything_is_launched(name):
    assert call("etp_pano_store_fwd", FWD_ARGS, **FWD_REFUSALS[name]) == -1, name
    assert b"etp_pano_store_fwd" in _lib.lib().etp_last_error()


@pytest.mark.parametrize("name", list(BWD_REFUSALS))
def test_bwd_refusals_come_back_before_anything_is_launched(name):
    assert call("etp_pano_store_bwd", BWD_ARGS, **BWD_REFUSALS[name]) == -1, name
    assert b"etp_pano_store_bwd" in _lib.lib().etp_last_error()


def _inputs(B=2, V=6, H=256, ks=(2, 1)):
    x = torch.zeros(B, V, H)
    masks = torch.ones(B, V, dtype=torch.bool)
    types = torch.zeros(B, V, dtype=torch.int64)
    for b, k in enumerate(ks):
        types[b, :k] = 1
    return x, masks, types, list(ks)


def test_embed_store_refuses_on_the_host_and_leaves_the_store_as_it_was():
    with pytest.raises(ValueError):
        EmbedStore(8, 384, "cpu")
    with pytest.raises(ValueError):
        EmbedStore(0, 256, "cpu")
    s = EmbedStore(8, 256, "cpu")
    assert s.rows_used == 0 and tuple(s.buf.shape) == (8, 256) and s.buf.dtype == torch.float32 and not s.buf.any()
    x, m, t, ks = _inputs()
    bad = [dict(pano_embeds=x.double()), dict(pano_embeds=x[:, :, :128]), dict(pano_embeds=x[0]), dict(pano_masks=m.float()),
           dict(pano_masks=m[:, :5]), dict(nav_types=t.int()), dict(nav_types=t[:1]), dict(n_cand=[2]), dict(n_cand=[2, 17]),
           dict(n_cand=[-1, 1]), dict(n_cand=[4, 4]),                                # 2 + 8 rows > capacity 8
           dict(pano_embeds=torch.zeros(2, 65, 256), pano_masks=torch.ones(2, 65, dtype=torch.bool), nav_types=torch.zeros(2, 65, dtype=torch.int64)),
           dict(pano_embeds=torch.zeros(2, 0, 256), pano_masks=torch.ones(2, 0, dtype=torch.bool), nav_types=torch.zeros(2, 0, dtype=torch.int64))]
    for kw in bad:
        a = dict(pano_embeds=x, pano_masks=m, nav_types=t, n_cand=ks)
        a.update(kw)
        with pytest.raises(ValueError):
            s.append(**a)
        assert s.rows_used == 0 and not s._blocks and not s._status and not s.buf.any()
    s.check()                                                 # nothing appended, nothing to copy


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_compute_fails_loudly_without_gpu():
    s = EmbedStore(8, 256, "cpu")
    x, m, t, ks = _inputs()
    with pytest.raises(_lib.EtpError):                        # valid input gets as far as the missing GPU
        s.append(x, m, t, ks)
    assert s.rows_used == 0 and not s._blocks
    maps = graph_inputs.DeviceGraphMaps(2, "cpu", False, 0.5, True, 0.0)
    with pytest.raises(_lib.EtpError):
        maps.img_fts(s, 4)
    with pytest.raises(_lib.EtpError):
        graph_inputs.gather_rows(s, [graph_inputs.GraphMapLite(False, 0.5, True, 0)], [0], 4)


def test_row_allocation_is_the_restatements():
    """episode b of a call gets 1 + n_cand[b] consecutive rows, in episode order, behind the rows used so far"""
    used = 5
    base, cand, used2 = pr.allocate(used, [2, 0, 16, 1])
    assert base.tolist() == [5, 8, 9, 26] and cand[0] == [6, 7] and cand[1] == [] and cand[2] == list(range(10, 26)) and cand[3] == [27]
    assert used2 == 28


def test_build_lists_the_file_with_the_row_kernel_flags():
    assert "pano_store.hip" in build.SOURCES and "pano_store.hip" in build.NO_PACKED_FP32 and "row.h" in build.HEADERS
    assert "-fno-slp-vectorize" in build.PER_SOURCE_FLAGS["pano_store.hip"]
    src = open(build.CSRC + "/pano_store.hip").read()
    assert "atomic" not in src.replace("no atomics", "") and "__shared__" not in src and '#include "row.h"' in src
    # the row idiom is shared, not copied
    assert "struct Row" not in src and "struct Row" not in open(build.CSRC + "/embed.hip").read()
    assert "struct Row" in open(build.CSRC + "/row.h").read()
