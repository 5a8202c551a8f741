"""Record which GEMM kernel instance the library launches for a list of products -> tests/golden/gemm_dispatch.json.

    python tools/record_gemm_dispatch.py --lib path/to/libetpnav_hip.so --commit <sha of that build> [--out FILE]

Needs the MI355X.  Every case is launched ONCE through etp_gemm / etp_gemm_group on zero-filled operands with the per-launch profiler
on, and the name the profiler reports is what the fixture keeps (or the refusal: return code + etp_last_error).  The library is the
one given by --lib -- a build of the commit the names are to be pinned to, never the code whose dispatch the fixture then checks
(tests/test_gemm_dispatch_cpu.py compares etp_gemm_instance against it on a machine without a GPU).

Cases:
  planner/*   every product the planner's linear_fwd / linear_fwd_s / linear_dgrad(_s) / linear_wgrad helpers (csrc/planner.hip) issue
              for one text layer, one panorama layer, one x-layer, the SAP head and the view projections, with the storage, C dtype,
              epilogue fields and split those helpers pass, at the row counts of BASELINE configs 2 (bf16 and fp32), 4 and 5; the grouped
              weight gradients of one text layer at 2560 and 8192 rows; the split-K dW[768,768].
  rule/*      per numeric rule of the selection two neighbouring shapes on either side of it: the recorder ASSERTS that their names
              differ (`pair`), so a pair that misses its threshold fails here, not in the test.
  forced/*    every value of every forcing switch x operand / C dtype x storage on a whole-tile and a ragged shape.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, I, IMG, DEP = 768, 3072, 512, 128            # hidden, intermediate, view feature sizes (oracle/planner_oracle.py PlannerConfig)


def planner_cases(gr):
    R = gr.dispatch_rec
    out = []

    def add(tag, recs, opts=None):
        out.append(dict(tag=tag, opts=opts or {}, descs=recs if isinstance(recs, list) else [recs]))

    def fwd(bf, M, N, K, ldy=None, act=gr.ACT_NONE):                               # linear_fwd
        return R(M, N, K, 0, 0, bf, bf, bias=True, act=act, Z=act not in (gr.ACT_NONE, gr.ACT_RELU), ldc=ldy or N)

    def fwd_s(bf, M, N, K, res=True):                                                # linear_fwd_s: fp32 C and residual
        return R(M, N, K, 0, 0, bf, False, bias=True, R=res)

    def dgrad(bf, M, N, K, ldy=None, act=gr.ACT_NONE):                             # linear_dgrad: dX[M,K] = dY[M,N] . W[N,K]
        return R(M, K, N, 0, 1, bf, bf, act=act, Z=act != gr.ACT_NONE, lda=ldy or N, ldb=K)

    def dgrad_s(bf, M, N, K, res=False, out_mode=0):                                 # linear_dgrad_s
        return R(M, K, N, 0, 1, bf, False, R=res, out_mode=out_mode, lda=N, ldb=K)

    def wgrad(bf, M, N, K, grouped, bias=True):                                      # linear_wgrad: dW[N,K] = dY[M,N]^T . X[M,K]
        bk = 64 if bf else 32
        dma = lambda ks: M % bk == 0 and M >= 2 * bk and M % ks == 0 and (M // ks) % bk == 0
        if grouped:
            return R(N, K, M, 1, 1, bf, False, out_mode=1, colsum=bias, lda=N, ldb=K)
        tiles = ((N + 63) // 64) * ((K + 63) // 64)
        ks = 4 if (tiles <= 144 and M >= 2048 and M % (4 * bk) == 0) else 1
        return R(N, K, M, 1, 1, bf, False, ksplit=ks, out_mode=2 if ks > 1 else 1, colsum=bias and dma(ks), lda=N, ldb=K)

    def layer(bf, M):            # self-attention projections + FFN of one transformer layer on M rows (text, panorama, x-layer node side)
        return [("qkv_fwd", fwd(bf, M, 3 * H, H)), ("attn_out_fwd", fwd_s(bf, M, H, H)),
                ("ffn_up_fwd", fwd(bf, M, I, H, act=gr.ACT_GELU_SAVEGRAD)), ("ffn_down_fwd", fwd_s(bf, M, H, I)),
                ("ffn_down_dgrad", dgrad(bf, M, H, I, act=gr.ACT_MUL_Z)), ("ffn_up_dgrad", dgrad_s(bf, M, I, H, res=True)),
                ("attn_out_dgrad", dgrad(bf, M, H, H)), ("qkv_dgrad", dgrad_s(bf, M, 3 * H, H, res=True)),
                ("ffn_down_wgrad", wgrad(bf, M, H, I, False)), ("ffn_up_wgrad", wgrad(bf, M, I, H, False)),
                ("attn_out_wgrad", wgrad(bf, M, H, H, False)), ("qkv_wgrad", wgrad(bf, M, 3 * H, H, False))]

    def text_group(bf, M):
        return [wgrad(bf, M, H, I, True), wgrad(bf, M, I, H, True), wgrad(bf, M, H, H, True), wgrad(bf, M, 3 * H, H, True)]

    # (config, bf16, text rows, panorama rows, graph rows)
    for cfg, bf, Mt, Mp, Mg in (("c2", True, 2560, 1152, 512), ("c2f32", False, 2560, 1152, 512), ("c4", True, 8192, 0, 0),
                                ("c5", True, 640, 288, 512)):
        for name, r in layer(bf, Mt):
            add(f"planner/{cfg}/text/{name}", r)
        if Mt in (2560, 8192):
            add(f"planner/{cfg}/text/wgrad_group", text_group(bf, Mt))
        if not Mp:
            continue
        for name, r in layer(bf, Mp):
            add(f"planner/{cfg}/pano/{name}", r)
        for name, r in (("img_fwd", fwd(bf, Mp, H, IMG)), ("dep_fwd", fwd(bf, Mp, H, DEP)), ("img_wgrad", wgrad(bf, Mp, H, IMG, False)),
                        ("dep_wgrad", wgrad(bf, Mp, H, DEP, False)), ("img_dgrad", dgrad_s(bf, Mp, H, IMG))):
            add(f"planner/{cfg}/view/{name}", r)
        for name, r in layer(bf, Mg):
            add(f"planner/{cfg}/x/{name}", r)
        for name, r in (("q_fwd", fwd(bf, Mg, H, H)), ("kv_fwd", fwd(bf, Mt, 2 * H, H)), ("xo_fwd", fwd_s(bf, Mg, H, H)),
                        ("xo_wgrad", wgrad(bf, Mg, H, H, False)), ("q_dgrad", dgrad_s(bf, Mg, H, H, res=True)),
                        ("kv_wgrad", wgrad(bf, Mt, 2 * H, H, False)), ("kv_dgrad", dgrad_s(bf, Mt, 2 * H, H, out_mode=1))):
            add(f"planner/{cfg}/x/{name}", r)
        for name, r in (("fwd", fwd(bf, Mg, H, H, act=gr.ACT_RELU)), ("wgrad", wgrad(bf, Mg, H, H, False)),
                        ("dgrad", dgrad_s(bf, Mg, H, H, res=True))):
            add(f"planner/{cfg}/sap/{name}", r)
    add("planner/splitk/dW768x768", wgrad(True, 2560, H, H, False))
    assert out[-1]["descs"][0]["ksplit"] == 4
    return out


def rule_cases(gr):
    R = gr.dispatch_rec
    out = []

    def pair(tag, a, b, opts=None, opts_b=None):
        for side, recs, o in (("a", a, opts), ("b", b, opts if opts_b is None else opts_b)):
            out.append(dict(tag=f"rule/{tag}/{side}", pair=f"rule/{tag}", opts=o or {}, descs=recs if isinstance(recs, list) else [recs]))

    def single(tag, rec, opts=None):
        out.append(dict(tag=f"rule/{tag}", opts=opts or {}, descs=[rec]))

    off = {"MM32": "0"}
    pair("mm32_128x128_at_320_tiles", R(2560, 2048, 256), R(2432, 2048, 256))
    pair("mm32_128x64_at_200_tiles", R(3200, 512, 256), R(3072, 512, 256))
    pair("gemm_128x128_at_360_tiles", R(2561, 2304, 256), R(2561, 2176, 256))
    pair("ring4_at_320_tiles", R(1280, 1024, 256), R(1344, 1024, 256))
    pair("ring4_at_4_slabs", R(1280, 1024, 256), R(1280, 1024, 192))
    pair("ring4_at_4_slabs_f32", R(1280, 1024, 128, bf16=False), R(1280, 1024, 96, bf16=False))
    for ta, tb in ((0, 0), (0, 1)):
        s = gr.sname(ta, tb)
        pair(f"32x64_at_128_tiles_{s}", R(512, 1024, 256, ta, tb), R(576, 1024, 256, ta, tb))
        pair(f"32x64_at_32_rows_{s}", R(32, 64, 256, ta, tb), R(31, 64, 256, ta, tb))
        pair(f"32x64_at_4_slabs_{s}", R(512, 1024, 256, ta, tb), R(512, 1024, 192, ta, tb))
    single("32x64_never_TN", R(512, 1024, 256, 1, 1, c_bf16=False))
    single("32x64_never_f32", R(512, 1024, 128, bf16=False))
    pair("32x64_switch", R(512, 1024, 256), R(512, 1024, 256), opts_b={"GEMM_SMALL": "0"})     # the same product, the class switched off
    for bf in (True, False):
        bk, t = (64, "bf16") if bf else (32, "f32")
        pair(f"dma_two_slabs_{t}", R(65, 72, 2 * bk, bf16=bf), R(65, 72, bk, bf16=bf), off)
        pair(f"dma_whole_slabs_{t}", R(65, 72, 2 * bk, bf16=bf), R(65, 72, 2 * bk + 8, bf16=bf), off)
        pair(f"dma_whole_slabs_per_split_{t}", R(136, 72, 4 * bk, 1, 1, bf, False, ksplit=2, out_mode=2),
             R(136, 72, 3 * bk, 1, 1, bf, False, ksplit=2, out_mode=2), off)
    G = lambda M, N, K: R(M, N, K, 1, 1, True, False)
    pair("group_128x128_at_160_tiles", [G(1280, 1024, 128), G(1280, 1024, 128)], [G(1280, 1024, 128), G(1152, 1024, 128)], off)
    pair("mm32_group_at_100_tiles", [G(640, 1280, 128), G(640, 1280, 128)], [G(640, 1280, 128), G(640, 1152, 128)])
    pair("mm32_group_256x128_at_kmin_4096", [G(2560, 1024, 4096), G(2560, 1024, 4096)], [G(2560, 1024, 4096), G(2560, 1024, 4032)])
    pair("mm32_group_256x128_at_160_tiles", [G(2560, 1024, 4096), G(2560, 1024, 4096)], [G(2560, 1024, 4096), G(2304, 1024, 4096)])
    # the windows of the classes that are off by default, under the switch that turns them on
    wide = {"MM32": "0", "GEMM_WIDE": "1"}
    pair("wide_at_200_tiles", R(3200, 512, 256), R(3072, 512, 256), wide)
    pair("wide_at_520_tiles", R(8320, 512, 256), R(8448, 512, 256), wide)
    pair("k2_at_256_tiles", R(2560, 768, 256), R(2816, 768, 256), {"MM32_K2": "264"})
    single("k2_keeps_64_class_TN", R(2560, 768, 256, 1, 1, c_bf16=False), {"MM32_K2": "264"})
    return out


FORCED = (("GEMM_TILE", ("32", "64", "64r", "64s2", "64s3", "64s4", "128", "128s3", "128r", "w", "ws2", "ws3", "256", "256s3")),
          ("MM32", ("0", "64", "128", "262", "264")), ("MM32_K2", ("262", "264")), ("GEMM_WIDE", ("1",)), ("GEMM_SMALL", ("0",)))
FORCED_GROUP = (("GROUP_TILE", ("64s3", "64s4", "128s2", "128s3", "256s2", "256s3")), ("MM32_GROUP", ("128", "256")))
DTYPES = ((True, True), (True, False), (False, False))         # (operands bf16, C bf16)


def forced_cases(gr):
    R = gr.dispatch_rec
    out = []
    for sw, values in FORCED:
        for v in values:
            for bf, cb in DTYPES:
                for ta, tb in gr.STOR:
                    for shape, (M, N, K) in (("whole", (2560, 768, 256)), ("ragged", (2561, 776, 192))):
                        opts = {sw: v}
                        if sw in ("GEMM_TILE", "GEMM_WIDE"):
                            opts["MM32"] = "0"              # (as _lib.force_gemm_tile does: the mm32 rules come first)
                        out.append(dict(tag=f"forced/{sw}={v}/{gr.tname(bf)},{gr.tname(cb)},{gr.sname(ta, tb)}/{shape}", opts=opts,
                                        descs=[R(M, N, K, ta, tb, bf, cb)]))
            if sw == "GEMM_TILE":                            # and with the mm32 rules left on, once per value: they still come first
                out.append(dict(tag=f"forced/{sw}={v}/mm32_on", opts={sw: v}, descs=[R(2560, 768, 256)]))
    for sw, values in FORCED_GROUP:
        for v in values:
            for bf, cb in DTYPES:
                for ta, tb in gr.STOR:
                    # whole 256x128 tiles | whole 128x128 tiles only | ragged, every member >= 128x128 but not >= 256x128 | a member below 128x128
                    for shape, members in (("whole", ((512, 256, 256), (256, 384, 512))), ("whole128", ((384, 256, 256), (128, 384, 512))),
                                           ("ragged", ((261, 136, 192), (130, 200, 256))), ("small", ((128, 128, 256), (64, 64, 128)))):
                        wgrad = bf and not cb and ta and tb                              # (the mm32 group rules see TN, fp32 C only)
                        # GROUP_TILE: gemm.hip's classes, mm32 off (and left on where its rules apply); MM32_GROUP: beside MM32=128, which
                        # takes every whole-tile group whatever its tile count (and with MM32 unset, where these small groups stay on gemm.hip)
                        for mm32 in (("0",) + ((None,) if wgrad else ())) if sw == "GROUP_TILE" else (("128", None) if wgrad else (None,)):
                            opts = {sw: v}
                            if mm32:
                                opts["MM32"] = mm32
                            out.append(dict(tag=f"forced/{sw}={v}/{gr.tname(bf)},{gr.tname(cb)},{gr.sname(ta, tb)}/{shape}"
                                                f"{('/mm32_off' if mm32 == '0' else '/mm32_' + mm32) if mm32 else ''}", opts=opts,
                                            descs=[R(M, N, K, ta, tb, bf, cb) for M, N, K in members]))
    return out


def all_cases(gr):
    cases = planner_cases(gr) + rule_cases(gr) + forced_cases(gr)
    tags = [c["tag"] for c in cases]
    assert len(tags) == len(set(tags)), "duplicate case tags"
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the library build whose dispatch is recorded")
    ap.add_argument("--commit", required=True, help="the commit that build was made from (kept in the fixture)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gemm_dispatch.json"))
    a = ap.parse_args()
    os.environ["ETP_LIB"] = os.path.abspath(a.lib)
    import torch
    from etpnav_amd import _lib
    from tests import gemm_ref as gr
    L = _lib.lib()
    cases = all_cases(gr)
    need = {"in": 1, "C": 1, "Z": 1}
    for c in cases:
        tot = {"C": 0, "Z": 0}
        for r in c["descs"]:
            e = gr.dispatch_extents(r)
            need["in"] = max(need["in"], 4 * max(e["A"], e["B"], e["R"], e["Z"], r["N"]))
            tot["C"] += 4 * e["C"] + 256
            tot["Z"] += 4 * e["Z"] + 256
        need["C"], need["Z"] = max(need["C"], tot["C"]), max(need["Z"], tot["Z"])
    zin = torch.zeros(need["in"], dtype=torch.uint8, device="cuda")              # every read-only operand: the same zeros
    bufC = torch.zeros(need["C"], dtype=torch.uint8, device="cuda")
    bufZ = torch.zeros(need["Z"], dtype=torch.uint8, device="cuda")
    bufS = torch.zeros(4 * 16384 * 8, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for c in cases:
        for k in gr.GEMM_SWITCHES:
            _lib.set_option(k, c["opts"].get(k))
        n = len(c["descs"])
        arr = (_lib.GemmDesc * n)()
        offC = offZ = 0
        for i, r in enumerate(c["descs"]):
            e = gr.dispatch_extents(r)
            at = {"A": zin.data_ptr(), "B": zin.data_ptr(), "bias": zin.data_ptr(), "R": zin.data_ptr(), "C": bufC.data_ptr() + offC,
                  "Z": (zin.data_ptr() if r["act"] in gr.ACT_READS_Z else bufZ.data_ptr() + offZ), "colsum": bufS.data_ptr() + 4 * 16384 * i}
            gr.dispatch_desc(arr[i], r, at.__getitem__)
            offC += (4 * e["C"] + 255) // 256 * 256
            offZ += (4 * e["Z"] + 255) // 256 * 256
        with _lib.profiled() as p:
            rc = L.etp_gemm(ctypes.byref(arr[0]), st) if n == 1 else L.etp_gemm_group(arr, n, st)
            torch.cuda.synchronize()
        if rc == 0:
            assert len(p.launches) == 1 and sum(p.launches.values()) == 1, (c["tag"], p.launches)
            c["name"] = next(iter(p.launches))
        else:
            assert p.launches == {}, (c["tag"], p.launches)
            c["rc"], c["error"] = rc, L.etp_last_error().decode()
    for k in gr.GEMM_SWITCHES:
        _lib.set_option(k, None)
    pairs = {}
    for c in cases:
        if "pair" in c:
            pairs.setdefault(c["pair"], []).append(c.get("name"))
    for k, names in pairs.items():
        assert len(names) == 2 and None not in names and names[0] != names[1], f"{k}: both sides ran {names}: the pair misses its threshold"
    with open(a.out, "w") as f:
        f.write('{"commit": %s,\n "recorded_with": "tools/record_gemm_dispatch.py",\n "cases": [\n' % json.dumps(a.commit))
        f.write(",\n".join("  " + json.dumps(dict(c, descs=[gr.dispatch_pack(r) for r in c["descs"]]), separators=(",", ":")) for c in cases))
        f.write("\n ]}\n")
    print(f"{len(cases)} cases ({len(pairs)} pairs, {sum(1 for c in cases if 'rc' in c)} refusals) from {a.commit} -> {a.out}")


if __name__ == "__main__":
    main()
