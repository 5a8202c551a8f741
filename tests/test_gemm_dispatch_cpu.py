"""Which GEMM kernel instance runs, asked on the host: etp_gemm_instance (include/etpnav_hip.h) goes through the launch's own argument
checks, the selection (csrc/gemm.hip: gemm_select / gemm_group_select) and the instance lists, and launches nothing -- so the choice is
tested here, without a GPU, on descriptors whose pointers are aligned fakes that are never dereferenced.

  * every instance tests/test_gemm_kernels_gpu.py lists (gemm_ref.REG / DMA / MM32 / GROUPS / MM32_GROUPS), under its own switches and
    at the shapes that file launches it with, is named exactly as listed -- which also shows that the library's lists hold it;
  * tests/golden/gemm_dispatch.json: names RECORDED ON THE MI355X from the library built at the commit the fixture states
    (tools/record_gemm_dispatch.py: each case launched once, the name read from the per-launch profiler) -- the planner's products at
    the workload's row counts, a pair of neighbouring shapes on either side of every numeric rule, every value of every forcing switch.
    The query reproduces every recorded name and every recorded refusal;
  * descriptor-level refusals: etp_gemm_instance and etp_gemm return the same code and leave the same etp_last_error (etp_gemm refuses
    before its first HIP call, as in test_boundary_cpu.py::test_argument_validation_without_launching)."""
import ctypes
import json
import os

import pytest

from etpnav_amd import _lib
from etpnav_amd._lib import GemmDesc
from tests import gemm_ref as gr

BF, F32 = _lib.ETP_BF16, _lib.ETP_F32
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_dispatch.json")
FAKE = {"A": 0x10000000, "B": 0x20000000, "C": 0x30000000, "bias": 0x40000000, "R": 0x50000000, "Z": 0x60000000, "colsum": 0x70000000}


def L():
    return _lib.lib()


def set_opts(etp_opt, opts):
    for k in gr.GEMM_SWITCHES:
        etp_opt(k, opts.get(k))


def query(descs):
    """-> the instance name, or (error code, etp_last_error) where the launch would refuse"""
    n = len(descs)
    arr = (GemmDesc * n)(*descs)
    buf = ctypes.create_string_buffer(96)
    rc = L().etp_gemm_instance(arr, n, buf, 96)
    if rc < 0:
        return rc, L().etp_last_error().decode()
    name = buf.value.decode()
    assert rc == len(name), (rc, name)
    assert "internal error" not in name
    return name


def fake(M, N, K, ta, tb, bf16, c_bf16, ld="pad", out_mode=0, colsum=False, slot=0):
    """the descriptor tests/test_gemm_kernels_gpu.py builds for such a product (its store() and out_layout(): operands with one spare
    16-byte chunk per row, C at column 8 of 16-byte aligned rows, or at column 3 of rows of odd length), over fake addresses"""
    epc = 8 if bf16 else 4
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.lda = gr.rup(M if ta else K, epc) + epc
    d.ldb = gr.rup(N if tb else K, epc) + epc
    d.ldc, col0 = (gr.rup(N, 8) + 64, 8) if ld == "pad" else (gr.rup(N, 8) + 61, 3)
    base = slot << 24
    d.A, d.B, d.C = FAKE["A"] + base, FAKE["B"] + base, FAKE["C"] + base + (2 * d.ldc + col0) * (2 if c_bf16 else 4)
    d.trans_a, d.trans_b, d.dtype, d.c_dtype = ta, tb, BF if bf16 else F32, BF if c_bf16 else F32
    d.batch, d.batch_inner, d.ksplit, d.alpha, d.out_mode = 1, 1, 1, 1.0, out_mode
    d.a_colsum = FAKE["colsum"] + base if colsum else None
    return d


@pytest.mark.parametrize("c", gr.SINGLES, ids=[c["name"] for c in gr.SINGLES])
def test_listed_instance_is_selected_at_its_shapes(c, etp_opt):
    """every (M, N, K) test_instance, the XCD test, the long-reduction test and the listing test launch this instance with, with
    16-byte aligned rows and (gemm.hip's kernels) with an odd leading dimension"""
    set_opts(etp_opt, c["opts"])
    shapes = set(gr.instance_shapes(c["kind"], c["bf16"], c["BM"], c["BN"], c["S"]))
    shapes |= {(2 * c["BM"], c["BN"], 72 if c["kind"] == "reg" else 256), (2 * c["BM"], c["BN"], 3072)}
    for M, N, K in sorted(shapes):
        for ld in ("pad",) if c["kind"].startswith("mm32") else ("pad", "odd"):
            got = query([fake(M, N, K, c["ta"], c["tb"], c["bf16"], c["c_bf16"], ld)])
            assert got == c["name"], (M, N, K, ld, got)


GROUPED = gr.GROUPS + gr.MM32_GROUPS


@pytest.mark.parametrize("c", GROUPED, ids=[c["name"] for c in GROUPED])
def test_listed_group_instance_is_selected_at_its_shapes(c, etp_opt):
    """test_groups' member lists (2, 5 and 8 problems, K in an order the launcher's sort changes and uniform) and the listing test's pair"""
    set_opts(etp_opt, c["opts"])
    bk = 64 if c["bf16"] else 32
    a = (c["ta"], c["tb"], c["bf16"], c["c_bf16"])
    for n in (2, 5, 8):
        for uniform in (False, True):
            Ks = [256 * bk // 64] * n if uniform else [k * bk // 64 for k in gr.GROUP_K[:n]]
            members = gr.group_members(c["BM"], c["BN"], c.get("whole", False), n)
            descs = [fake(M, N, K, *a, out_mode=i % 2, colsum=bool(c["ta"] and c["tb"] and i % 2 == 0), slot=i)
                     for i, ((M, N), K) in enumerate(zip(members, Ks))]
            assert query(descs) == c["name"], (n, uniform)
    assert query([fake(2 * c["BM"], c["BN"], 256, *a, slot=i) for i in range(2)]) == c["name"]


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert len(fx["commit"]) == 40, "the fixture states the commit its names were recorded from"
    return fx["cases"]


def test_recorded_dispatch_is_reproduced(recorded, etp_opt):
    """every case of the fixture: the same switches, the same descriptor fields -> the recorded name (or the recorded refusal)"""
    assert len(recorded) >= 300
    wrong = []
    for c in recorded:
        set_opts(etp_opt, c["opts"])
        descs = [gr.dispatch_desc(GemmDesc(), gr.dispatch_unpack(r), lambda k, i=i: FAKE[k] + (i << 24)) for i, r in enumerate(c["descs"])]
        got = query(descs)
        want = c["name"] if "name" in c else (c["rc"], c["error"])
        if got != want:
            wrong.append((c["tag"], want, got))
    assert not wrong, f"{len(wrong)} of {len(recorded)} cases, the first: {wrong[:5]}"


def test_fixture_covers_the_workload_the_rules_and_the_forced_forms(recorded):
    tags = {c["tag"]: c for c in recorded}
    for cfg, rows in (("c2", 2560), ("c2f32", 2560), ("c4", 8192), ("c5", 640)):
        assert tags[f"planner/{cfg}/text/ffn_up_fwd"]["descs"][0]["M"] == rows
    assert {tags[t]["descs"][0]["M"] for t in ("planner/c2/pano/qkv_fwd", "planner/c2/x/qkv_fwd", "planner/c5/pano/qkv_fwd")} == {1152, 512, 288}
    for t in ("planner/c2/text/wgrad_group", "planner/c4/text/wgrad_group"):
        assert len(tags[t]["descs"]) == 4 and tags[t]["name"].startswith("mm32_group<")
    assert tags["planner/splitk/dW768x768"]["descs"][0]["ksplit"] == 4
    pairs = {}
    for c in recorded:
        if "pair" in c:
            pairs.setdefault(c["pair"], []).append(c["name"])
    assert len(pairs) >= 20 and all(len(v) == 2 and v[0] != v[1] for v in pairs.values()), pairs
    forced = {t.split("/")[1] for t in tags if t.startswith("forced/")}
    want = {f"GEMM_TILE={v}" for v in ("32", "64", "64r", "64s2", "64s3", "64s4", "128", "128s3", "128r", "w", "ws2", "ws3", "256", "256s3")}
    want |= {f"GROUP_TILE={v}" for v in ("64s3", "64s4", "128s2", "128s3", "256s2", "256s3")}
    want |= {f"MM32={v}" for v in ("0", "64", "128", "262", "264")} | {"MM32_GROUP=128", "MM32_GROUP=256", "MM32_K2=262", "MM32_K2=264",
                                                                      "GEMM_WIDE=1", "GEMM_SMALL=0"}
    assert forced == want, (sorted(want - forced), sorted(forced - want))
    # the fallbacks the selection spells out, pinned to what the recorded library ran
    assert tags["forced/GEMM_TILE=64s2/bf16,bf16,NT/whole"]["name"] == "gemm_dma<bf16,bf16,NT,64x64,s3>"
    assert tags["forced/GEMM_TILE=256s3/f32,f32,NT/whole"]["name"] == "gemm_dma<f32,f32,NT,128x128,s3>"
    assert tags["forced/GEMM_TILE=256/f32,f32,TN/ragged"]["name"] == "gemm_dma<f32,f32,TN,128x128,s2>"
    assert tags["forced/MM32=264/bf16,f32,TN/whole"]["name"] == "mm32<bf16,f32,TN,128x64,s3>"
    assert tags["rule/k2_keeps_64_class_TN"]["name"] == "mm32<bf16,f32,TN,128x64,s3>"
    assert tags["forced/GROUP_TILE=256s2/bf16,f32,TN/small/mm32_off"]["name"] == "gemm_group<bf16,f32,TN,64x64,s3>"
    assert tags["forced/GROUP_TILE=128s2/bf16,f32,TN/small/mm32_off"]["name"] == "gemm_group<bf16,f32,TN,64x64,s3>"
    assert tags["forced/GROUP_TILE=256s3/bf16,f32,TN/ragged/mm32_off"]["name"] == "gemm_group<bf16,f32,TN,64x64,s3>"
    assert tags["forced/MM32_GROUP=256/bf16,f32,TN/whole/mm32_128"]["name"] == "mm32_group<bf16,f32,TN,256x128,s3>"
    assert tags["forced/MM32_GROUP=256/bf16,f32,TN/whole128/mm32_128"]["name"] == "mm32_group<bf16,f32,TN,128x128,s2>"
    assert tags["forced/MM32_GROUP=128/bf16,f32,TN/whole/mm32_128"]["name"] == "mm32_group<bf16,f32,TN,128x128,s2>"


def plain(M=64, N=64, K=128, ta=0, tb=0, bf16=True, c_bf16=None):
    c_bf16 = bf16 if c_bf16 is None else c_bf16
    d = fake(M, N, K, ta, tb, bf16, c_bf16)
    d.C, d.ldc = FAKE["C"], N
    return d


def test_refusals_are_the_launch_entry_points_own():
    """the descriptor-level refusals of test_gemm_kernels_gpu.py::test_refusals: the query and the launch entry point return the same
    code and leave the same message, and neither touches the GPU"""
    def both(descs, what, word):
        n = len(descs)
        arr = (GemmDesc * n)(*descs)
        q = query(list(arr))
        rc = L().etp_gemm(ctypes.byref(arr[0]), None) if n == 1 else L().etp_gemm_group(arr, n, None)
        assert isinstance(q, tuple) and q == (rc, L().etp_last_error().decode()) and rc == -1, (what, q, rc, L().etp_last_error())
        assert word in q[1], (what, q)

    def mod(d, **kw):
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    both([mod(plain(), M=0)], "bad dims", "bad dims")
    both([mod(plain(), ksplit=1, batch_inner=1, K=-8)], "negative K", "bad dims")
    d = plain()
    both([mod(d, lda=d.lda + 4)], "misaligned lda", "16-byte chunk")
    both([mod(plain(), A=FAKE["A"] + 2)], "misaligned A", "16-byte aligned")
    both([mod(plain(c_bf16=False), ksplit=2)], "split without atomics", "split-K needs atomic")
    both([mod(plain(), out_mode=2)], "atomics into a bf16 C", "fp32 C")
    both([mod(plain(bf16=False), c_dtype=BF)], "fp32 operands with a bf16 C", "fp32 operands need an fp32 C")
    both([mod(plain(c_bf16=False), a_colsum=FAKE["colsum"])], "a_colsum on an NT product", "a_colsum")
    both([mod(plain(K=72, ta=1, tb=1, c_bf16=False), a_colsum=FAKE["colsum"])], "a_colsum off the LDS-DMA kernel", "a_colsum")
    both([plain(ta=1, tb=0)], "(A trans, B row) storage", "storage pairing")
    both([mod(plain(), act=gr.ACT_GELU)], "activation without Z", "activation needs Z")
    both([mod(plain(), A=None)], "null operand", "null")
    for split in (True, False):
        how = dict(ksplit=2, out_mode=2) if split else dict(batch=2, batch_inner=1)
        both([mod(plain(c_bf16=False), R=FAKE["R"], ldr=64, **how)], "R on a split / batched product", "unsplit, unbatched")
        both([mod(plain(c_bf16=False), Z=FAKE["Z"], ldz=64, **how)], "Z on a split / batched product", "unsplit, unbatched")
        both([mod(plain(c_bf16=False), act=gr.ACT_RELU, **how)], "activation on a split / batched product", "unsplit, unbatched")
    pair = lambda: [plain(64, 64, 128, 1, 1, c_bf16=False), plain(64, 64, 128, 1, 1, c_bf16=False)]
    g = pair(); g[1].K = 64
    both(g, "group: a member shorter than two slabs", "LDS-DMA-able")
    g = pair(); g[0].ksplit, g[0].out_mode = 2, 2
    both(g, "group: a split member", "unbatched, unsplit")
    g = pair(); g[1].batch = 2
    both(g, "group: a batched member", "unbatched, unsplit")
    g = pair(); g[1].dtype = F32
    both(g, "group: mixed operand dtypes", "share dtype")
    g = pair(); g[1].trans_a = 0
    both(g, "group: mixed storage classes", "share dtype")
    both([plain(64, 64, 128, 1, 1, c_bf16=False) for _ in range(9)], "group: n = 9", "1..8 descriptors")
    assert L().etp_gemm_instance(None, 1, None, 0) == -1 and L().etp_gemm_instance(None, 2, None, 0) == -1
    assert L().etp_gemm_instance(ctypes.byref(plain()), 0, None, 0) == -1


def test_name_is_truncated_to_cap_and_its_length_returned():
    d = plain(65, 72, 72)
    full = query([d])
    assert full == "gemm<bf16,bf16,NT,64x64,s0>"
    buf = ctypes.create_string_buffer(b"#" * 16, 16)
    assert L().etp_gemm_instance(ctypes.byref(d), 1, buf, 8) == len(full)
    assert buf.raw[:8] == full[:7].encode() + b"\0" and buf.raw[8:] == b"#" * 8
    assert L().etp_gemm_instance(ctypes.byref(d), 1, None, 0) == len(full)
