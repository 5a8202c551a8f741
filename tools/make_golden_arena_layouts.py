"""Snapshot of every engine's parameter-arena layout and scratch sizes -> tests/golden/arena_layouts.json.

    python tools/make_golden_arena_layouts.py            # rewrite the fixture from the built library (no GPU needed)

tests/test_arena_layout_cpu.py recomputes `snapshot()` from the current build and compares it for equality: the 64-element offset rule,
the region order and the 256-byte scratch granule are what the fused AdamW, the data-parallel slice plan and every caller-sized buffer
rely on.  Everything goes through the C ABI directly, not through the Python modules, so the snapshot does not move with them.
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "arena_layouts.json")

BATCHES = (1, 3)
TEXT_LENGTHS = (5, 80)
V, G, NM = 3, 4, 2
PLANNER_QUERIES = {"etp_txt_stash_bytes": "BL", "etp_txt_ws_bytes": "BL", "etp_pano_stash_bytes": "BV", "etp_pano_ws_bytes": "BV",
                   "etp_nav_stash_bytes": "BLG", "etp_nav_ws_bytes": "BLG", "etp_nav_kv_bytes": "BL", "etp_nav_kv_offset": "BL",
                   "etp_mlm_stash_bytes": "BLGN", "etp_mlm_ws_bytes": "BLGN"}


def _layout(L, prefix, h, info, full):
    rows = []
    for i in range(getattr(L, f"etp_{prefix}_param_count")(h)):
        rc = getattr(L, f"etp_{prefix}_param_info")(h, i, ctypes.byref(info))
        assert rc == 0, (prefix, i, L.etp_last_error())
        shape = "x".join(str(int(info.shape[k])) for k in range(info.ndim))
        rows.append(f"{info.name.decode()}|{shape}|{int(info.offset)}")
    out = {"count": len(rows), "total": int(getattr(L, f"etp_{prefix}_arena_elems")(h)),
           "n_matrix": int(getattr(L, f"etp_{prefix}_matrix_elems")(h)),
           "sha256": hashlib.sha256("\n".join(rows).encode()).hexdigest()}
    if full:
        out["table"] = rows
    return out


def snapshot() -> dict:
    import torch
    from etpnav_amd import _lib
    from etpnav_amd.planner import default_config, make_c_config
    L = _lib.lib()
    dts = {"f32": (_lib.ETP_F32, torch.float32), "bf16": (_lib.ETP_BF16, torch.bfloat16)}
    snap = {}
    for lang2visn in (False, True):
        for dname, (_, tdt) in dts.items():
            c = make_c_config(default_config("r2r", use_lang2visn_attn=lang2visn), tdt)
            h = L.etp_planner_create(ctypes.byref(c))
            assert h, L.etp_last_error()
            try:
                e = _layout(L, "planner", h, _lib.ParamInfo(), full=False)
                e["bytes"] = {}
                for B in BATCHES:
                    for Lt in TEXT_LENGTHS:
                        dims = {"B": B, "L": Lt, "V": V, "G": G, "N": NM}
                        e["bytes"][f"B{B}_L{Lt}"] = {fn: int(getattr(L, fn)(h, *(dims[d] for d in sig)))
                                                     for fn, sig in PLANNER_QUERIES.items() if lang2visn or not fn.startswith("etp_mlm")}
                snap[f"planner/r2r{'+lang2visn' if lang2visn else ''}/{dname}"] = e
            finally:
                L.etp_planner_destroy(h)
    for dname, (edt, _) in dts.items():
        h = L.etp_waypoint_create(edt)
        assert h, L.etp_last_error()
        try:
            e = _layout(L, "waypoint", h, _lib.ParamInfo(), full=True)
            e["bytes"] = {f"B{B}": int(L.etp_waypoint_ws_bytes(h, B)) for B in BATCHES}
            snap[f"waypoint/{dname}"] = e
        finally:
            L.etp_waypoint_destroy(h)
        for S, layers in ((224, 12), (64, 2)):
            h = L.etp_clip_create(edt, S, layers)
            assert h, L.etp_last_error()
            try:
                e = _layout(L, "clip", h, _lib.ClipTensorInfo(), full=S == 64)
                e["bytes"] = {f"N{N}": int(L.etp_clip_ws_bytes(h, N)) for N in BATCHES}
                snap[f"clip/{S}x{layers}/{dname}"] = e
            finally:
                L.etp_clip_destroy(h)
        for S, bp, blocks in ((256, 32, (3, 4, 6, 3)), (64, 16, (1, 1, 1, 1))):
            h = L.etp_depth_create(edt, S, bp, (ctypes.c_int * 4)(*blocks))
            assert h, L.etp_last_error()
            try:
                e = _layout(L, "depth", h, _lib.DepthTensorInfo(), full=S == 64)
                e["out_channels"] = int(L.etp_depth_out_channels(h))
                e["bytes"] = {f"N{N}": int(L.etp_depth_ws_bytes(h, N)) for N in BATCHES}
                snap[f"depth/{S}x{bp}x{'-'.join(map(str, blocks))}/{dname}"] = e
            finally:
                L.etp_depth_destroy(h)
    return snap


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(snapshot(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
