"""The multi-stream step schedule, replayed in every order its recorded graph allows.

A training step is issued on up to four streams tied together by ~80 event edges (step.py, pretrain.py, planner.hip).  A missing edge
is a race that no result test at B = 4 sees: the consumer still runs after its producer by luck.  Here the step is RECORDED
(etp_rec_begin / etp_rec_end), and the recorded partial order is then replayed as plain chain graphs (etp_graph_linearize), one per
logical stream k: the linear extension that emits stream k as late as possible (tests/sched_ref.py; pinned without a GPU by
tests/test_sched_ref_cpu.py).  Over the S extensions every pair of nodes the graph leaves unordered runs in both orders.  Every buffer
the step owns is filled with 0xFF bytes before each replay, so

    a read before its write   -> NaN in the loss, an output or a gradient,
    a write after a read or a second write in the wrong order -> a wrong value,

on the first run, deterministically, with no race actually happening: a chain graph has no parallel branches.

Fidelity (per recorded graph): the closure of the edges the HIP runtime reports (hipGraphGetEdges) equals the happens-before relation
of the independent stream / event model over the recorder's call trace; the kernel-node count equals what etp_rec_end reported; every
node lies on exactly one stream; a whole step ends joined (whatever is issued next on the origin stream is ordered after every node;
see check_fidelity for why this is stated on the stream's frontier and not on its last node).

Order independence: the reference is the same step issued eagerly on ONE stream (overlap=False) from the same 0xFF-filled state.  Per
tensor (every output / gradient-side API tensor, every trainable parameter's gradient slice): the same elements are written, no NaN
among them, |got - ref| <= tol * max(1, max|ref|) with the recorded-graph test's tol (1e-4 fp32, 2e-3 bf16), loss within 1e-5, and a
tensor that is all zero in the reference stays all zero.  Gradient slots of frozen parameters are unspecified and left out.

Safety of the method: a wrong order can only produce wrong NUMBERS as long as no kernel takes an address or an index from a buffer the
step itself produces.  The stash and workspace layouts (planner.hip plan_txt / plan_pano / plan_nav / plan_mlm and their *_ws twins) hold
fp32 / bf16 activations and statistics only, plus one byte mask (PanoStash::mask; the API tensor pmask is its twin), for which 0xFF is a
legal value; index arrays (CSR, token ids, labels, the MLM row selections) are inputs and are not poisoned.

The two toy programs at the end are deliberately under-synchronised.  They are only recorded and only replayed as chains (never issued
eagerly, never launched as the parallel graph): the checker must flag each, and neither of their correctly joined twins.
"""
import ctypes
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import planner_oracle as po  # noqa: E402  (parameters and batches only)
from tests import sched_ref as sr  # noqa: E402
from etpnav_amd import _lib  # noqa: E402
from etpnav_amd._lib import check, ptr  # noqa: E402
from etpnav_amd.planner import GlocalTextPathNavCMT  # noqa: E402
from etpnav_amd.step import PlannerStep, MicroBatchedStep  # noqa: E402

RATES = (0.1, 0.1, 0.1, 0.4)
SEED = 7
_T = {"t0": time.time()}                     # reset when the module's first test starts (the `stream` fixture)


def _elapsed():
    return time.time() - _T["t0"]


REPORT = os.environ.get("ETP_SCHED_REPORT")          # a file that receives one line per case (profiles/sched_orders.txt)


# ---- recording any callable, and the recorder's introspection -------------------------------------------------------------------------
class Recorded:
    """One graph recorded from `fn(stream)` (or a chain built from one), with what the library tells about it."""

    def __init__(self, L, handle, n_kernels=None, n_edges=None):
        self.L, self.h, self.n_kernels, self.n_edges = L, handle, n_kernels, n_edges
        out = (ctypes.c_int64 * 4)()
        check(L.etp_graph_info(self.h, out), "graph_info")
        self.n, self.n_rows, self.n_rt_edges, self.n_streams = (int(x) for x in out)
        rows = (ctypes.c_int32 * (4 * max(self.n_rows, 1)))()
        check(L.etp_graph_trace(self.h, rows, self.n_rows), "graph_trace")
        self.trace = [tuple(rows[4 * i:4 * i + 4]) for i in range(self.n_rows)]
        f, t = (ctypes.c_int32 * max(self.n_rt_edges, 1))(), (ctypes.c_int32 * max(self.n_rt_edges, 1))()
        check(L.etp_graph_edges(self.h, f, t, self.n_rt_edges), "graph_edges")
        self.edges = [(int(f[i]), int(t[i])) for i in range(self.n_rt_edges)]

    def name(self, i):
        buf = ctypes.create_string_buffer(256)
        check(self.L.etp_graph_node_name(self.h, i, buf, 256), "graph_node_name")
        return buf.value.decode()

    def chain(self, order):
        arr = (ctypes.c_int32 * len(order))(*order)
        g = ctypes.c_void_p()
        check(self.L.etp_graph_linearize(self.h, arr, len(order), ctypes.byref(g)), "graph_linearize")
        return Recorded(self.L, g.value)

    def launch(self, stream):
        check(self.L.etp_graph_launch(self.h, stream), "graph_launch")

    def destroy(self):
        if self.h:
            self.L.etp_graph_destroy(self.h)
            self.h = None


def record(L, fn, stream):
    """etp_rec_begin, fn(stream), etp_rec_end: works for any callable that issues library calls (PlannerStep, MlmStep,
    MicroBatchedStep, the toy programs) without a change to them"""
    check(L.etp_rec_begin(), "rec_begin")
    try:
        fn(stream)
    except Exception:
        L.etp_rec_abort()
        raise
    g, nk, ne = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
    check(L.etp_rec_end(ctypes.byref(g), ctypes.byref(nk), ctypes.byref(ne)), "rec_end")
    return Recorded(L, g.value, int(nk.value), int(ne.value))


@pytest.fixture(scope="module")
def stream():
    L = _lib.lib()
    _T["t0"] = time.time()
    s = ctypes.c_void_p()
    check(L.etp_stream_create(ctypes.byref(s)), "stream_create")
    yield s.value
    torch.cuda.synchronize()
    L.etp_stream_destroy(s.value)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(f"tests/test_sched_gpu.py: wall time {_elapsed():.1f} s on the MI355X\n")


# ---- fidelity ---------------------------------------------------------------------------------------------------------------------------
def check_fidelity(rec, whole_step):
    anc = sr.hb_closure(rec.trace)
    assert len(anc) == rec.n == sr.n_nodes(rec.trace)
    got = sr.graph_closure(rec.n, rec.edges)
    if got != anc:
        x = next(i for i in range(rec.n) if got[i] != anc[i])
        lost = [j for j in range(rec.n) if (anc[x] & ~got[x]) >> j & 1]
        extra = [j for j in range(rec.n) if (got[x] & ~anc[x]) >> j & 1]
        raise AssertionError(f"node {x} ({rec.name(x)}): the runtime's graph lacks ancestors {[(j, rec.name(j)) for j in lost[:4]]}, "
                             f"has {[(j, rec.name(j)) for j in extra[:4]]} beyond the stream / event model")
    kinds = [r[0] for r in rec.trace if r[0] in (sr.KERNEL, sr.MEMSET, sr.JOIN)]
    assert kinds.count(sr.KERNEL) == rec.n_kernels                      # graph_stats' kernel count
    streams = sr.node_streams(rec.trace)                                 # raises unless every node index occurs exactly once, in order
    assert len(streams) == rec.n and len(set(r[1] for r in rec.trace)) == rec.n_streams
    if whole_step:
        # The step ends joined: whatever is issued next on the origin stream is ordered after every node.  Where a node follows the
        # closing join this is "every node is an ancestor of the origin stream's last node"; the steps close with waits that no node
        # follows (etp_stream_after(s2, s) at the end of enqueue_txt_bwd), which live in the stream's state and not in the graph, so the
        # statement is made on the model's frontier of the origin stream.
        origin = rec.trace[0][1]                                         # every step starts on the stream it was given
        front = sr.stream_frontiers(rec.trace)[origin]
        assert front == (1 << rec.n) - 1, \
            f"the step does not end joined: {[rec.name(x) for x in range(rec.n) if not (front >> x) & 1][:6]}"
    return anc, streams


# ---- order independence -----------------------------------------------------------------------------------------------------------------
def poison(tensors):
    for t in tensors:
        t.view(torch.uint8).fill_(0xFF)


def compare(name, got, ref, tol):
    """-> (problem or None, |err| / tolerance) for one tensor against the single-stream reference"""
    if got.dtype in (torch.bool, torch.uint8):
        bad = int((got.view(torch.uint8) != ref.view(torch.uint8)).sum())
        return (f"{name}: {bad} bytes differ" if bad else None), 0.0
    got, ref = got.float().reshape(-1), ref.float().reshape(-1)
    if not torch.equal(got.isnan(), ref.isnan()):
        return f"{name}: {int((got.isnan() & ~ref.isnan()).sum())} NaN where the reference has numbers, " \
               f"{int((~got.isnan() & ref.isnan()).sum())} numbers where the reference left the fill", float("inf")
    w = ~ref.isnan()
    got, ref = got[w], ref[w]
    inf = ref.isinf()
    if not torch.equal(got[inf], ref[inf]) or bool(got[~inf].isinf().any()):
        return f"{name}: infinities differ", float("inf")
    got, ref = got[~inf], ref[~inf]
    if ref.numel() == 0:
        return None, 0.0
    amax = float(ref.abs().max())
    err = float((got - ref).abs().max())
    if amax == 0.0 and err != 0.0:
        return f"{name}: all zero in the reference, max |value| {err:.3e} here", float("inf")
    bound = tol * max(1.0, amax)
    return (f"{name}: max |err| {err:.3e} > {bound:.3e}" if err > bound else None), err / bound


def snapshot(tensors):
    return {k: v.detach().clone() for k, v in tensors.items()}


def grad_slices(model):
    """trainable parameters' slices of the flat gradient arena, by name"""
    eng = model._engine
    return {"grad " + name: eng.grads[off:off + n] for (p, off, n, _), (name, _, _) in zip(model._views, eng.table) if p.requires_grad}


def run_orders(recs, stream, owned, outputs, ref, tol):
    """Replay the recorded graph(s) `recs` (launched back to back) in every extension (every combination of extensions for several
    graphs) from a 0xFF-filled state.  -> (failures, number of replays, worst |err| / tolerance)"""
    fams = []
    for rec in recs:
        exts = sr.extensions(rec.trace)
        anc = sr.hb_closure(rec.trace)
        assert all(sr.is_extension(anc, o) for o in exts) and sr.uncovered_pairs(anc, exts) == []
        fams.append([(k, rec.chain(o)) for k, o in enumerate(exts)])
    combos = [[]]
    for fam in fams:
        combos = [c + [m] for c in combos for m in fam]
    failures, worst = [], 0.0
    try:
        for combo in combos:
            poison(owned)
            torch.cuda.synchronize()
            for _k, chain in combo:
                chain.launch(stream)
            check(_lib.lib().etp_stream_sync(stream), "stream_sync")
            torch.cuda.synchronize()
            tag = "late stream " + "/".join(str(k) for k, _ in combo)
            for name, t in outputs.items():
                bad, ratio = compare_loss(name, t, ref[name]) if name.endswith("loss") else compare(name, t, ref[name], tol)
                worst = max(worst, ratio if ratio != float("inf") else 0.0)
                if bad:
                    failures.append(f"[{tag}] {bad}")
    finally:
        for fam in fams:
            for _k, chain in fam:
                chain.destroy()
    return failures, len(combos), worst


def compare_loss(name, got, ref):
    g, r = float(got.reshape(-1)[0]), float(ref.reshape(-1)[0])
    if g != g or r != r:
        return f"{name}: NaN ({g} against {r})", float("inf")
    return (f"{name}: {g!r} against {r!r}" if abs(g - r) >= 1e-5 else None), abs(g - r) / 1e-5


def report(case, recs, n_runs, worst):
    line = f"{case}: " + " + ".join(
        f"{r.n_streams} streams {r.n} nodes {r.n_rt_edges} edges {sr.incomparable_pairs(sr.hb_closure(r.trace))} incomparable pairs"
        for r in recs) + f"; {n_runs} orders run; worst |err| / tolerance {worst:.3g}; file wall time so far {_elapsed():.1f} s"
    print(line)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(line + "\n")


# ---- models and steps -------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def model_for(dtype, **cfg_kw):
    key = (dtype, tuple(sorted(cfg_kw.items())))
    if key not in _MODELS:
        cfg = po.PlannerConfig.r2r(vocab_size=4096, **cfg_kw)
        m = GlocalTextPathNavCMT(cfg.to_dict(), dtype=dtype, device="cuda")
        m.load_state_dict(po.init_params(cfg, seed=11), strict=True)
        _MODELS[key] = (cfg, m.eval())
    return _MODELS[key]


def planner_owned(step):
    eng = step.eng
    own = [step.st_txt, step.st_pano, step.st_nav, step.ws_txt, step.ws_pano, step.ws_nav, eng.grads]
    if eng.shadow is not None:
        own.append(eng.shadow)
    api = {"txt": step.txt, "pano": step.pano, "pmask": step.pmask, "gimg": step.gimg, "gemb": step.gemb, "logits": step.logits,
           "dlogits": step.dlogits, "d_txt": step.d_txt, "d_gimg": step.d_gimg, "d_pano": step.d_pano, "loss": step.loss}
    return own + list(api.values()), api


def reference_planner(model, batch, parts=1):
    """the same step eagerly on ONE stream (overlap=False), from the same 0xFF-filled state; `parts` > 1: the micro-batches one after
    the other, as MicroBatchedStep builds them"""
    B = batch["txt_ids"].shape[0]
    mb = B // parts
    steps = []
    for k in range(parts):
        sub = batch if parts == 1 else {key: (v[k * mb:(k + 1) * mb] if torch.is_tensor(v) and v.shape[:1] == (B,) else v)
                                        for key, v in batch.items()}
        st = PlannerStep(model, sub, overlap=False, dropout=RATES, drop_seed=SEED * parts + k if parts > 1 else SEED,
                         refresh_weights=(k == 0), zero_grads=(k == 0), grad_overwrite=(None if k == 0 else False))
        st.loss_scale = 1.0 / B
        steps.append(st)
    owned, api = [], {}
    for k, st in enumerate(steps):
        o, a = planner_owned(st)
        owned += o
        api.update({(f"part{k} " if parts > 1 else "") + n: t for n, t in a.items()})
    poison(owned)
    torch.cuda.synchronize()
    if parts == 1:
        steps[0].run_eager()
    else:                                        # MicroBatchedStep.run_eager's issue order, on one stream
        s = steps[0].eng.stream()
        for st in steps:
            st.enqueue_fwd(s, True)
        for st in steps:
            st.enqueue_bwd_main(s, join_pano=False)
        for st in steps:
            st.enqueue_txt_bwd(s)
    torch.cuda.synchronize()
    ref = snapshot({**api, **grad_slices(model)})
    for st in steps:
        st.close()
    for name, t in ref.items():
        if name.startswith("grad ") or name.endswith("loss"):
            assert not bool(t.isnan().any()), f"the single-stream reference left {name} unwritten"
    return ref


CASES = {
    #                  dtype            overlap  environment                      config              batch (B, L)   how
    "default_fp32":   (torch.float32,  True,    {},                              {},                 (4, 33),      "step"),
    "default_bf16":   (torch.bfloat16, True,    {},                              {},                 (4, 33),      "step"),
    "chain_first":    (torch.bfloat16, True,    {"ETP_CHAIN_FIRST": "1"},        {},                 (4, 33),      "step"),
    "txt_cast_whole": (torch.bfloat16, True,    {"ETP_TXT_CAST_SPLIT": "0"},     {},                 (4, 33),      "step"),
    "assemble_main":  (torch.bfloat16, True,    {"ETP_ASSEMBLE_ON_S2": "0"},     {},                 (4, 33),      "step"),
    "no_dtxt_stream": (torch.bfloat16, True,    {"ETP_DTXT_STREAM": "0"},        {},                 (4, 33),      "step"),
    "overlap_aux":    (torch.bfloat16, "aux",   {},                              {},                 (4, 33),      "step"),
    "overlap_s2":     (torch.bfloat16, "s2",    {},                              {},                 (4, 33),      "step"),
    "split_text_bwd": (torch.bfloat16, True,    {},                              {},                 (4, 33),      "split"),
    "data_parallel":  (torch.bfloat16, True,    {},                              {},                 (4, 33),      "dp"),
    "fix_lang":       (torch.bfloat16, True,    {},  {"fix_lang_embedding": True},                   (4, 33),      "step"),
    "fix_pano":       (torch.bfloat16, True,    {},  {"fix_pano_embedding": True},                   (4, 33),      "step"),
    "fix_both":       (torch.bfloat16, True,    {},  {"fix_lang_embedding": True, "fix_pano_embedding": True}, (4, 33), "step"),
    # batch * heads = 288 > 256 CUs and Lq = 80 > 64: the attention backward leaves the folded out-projection, other launches
    "b24_l80":        (torch.bfloat16, True,    {},                              {},                 (24, 80),     "step"),
    "l160_streaming": (torch.bfloat16, True,    {},                              {},                 (4, 160),     "step"),
    "micro_batched":  (torch.bfloat16, True,    {},                              {},                 (4, 33),      "micro"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_recorded_step_is_order_independent(case, stream, monkeypatch):
    dtype, overlap, env, cfg_kw, (B, Lt), how = CASES[case]
    L = _lib.lib()
    cfg, model = model_for(dtype, **cfg_kw)
    batch = po.make_batch(cfg, B=B, L=Lt, V=19, G=10, seed=99, ragged=True)
    tol = 1e-4 if dtype == torch.float32 else 2e-3
    ref = reference_planner(model, batch, parts=2 if how == "micro" else 1)
    for k, v in env.items():                     # the switches are read once, in PlannerStep.__init__
        monkeypatch.setenv(k, v)
    if how == "micro":
        step = MicroBatchedStep(model, batch, n_micro=2, dropout=RATES, drop_seed=SEED)
        parts = step.parts
    else:
        step = PlannerStep(model, batch, overlap=overlap, dropout=RATES, drop_seed=SEED)
        parts = [step]
    try:
        for p in parts:
            p.step_no = -1                       # warm-up run = step 0, the recorded step = step 1: the reference's masks
        step.run_eager()
        torch.cuda.synchronize()
        if how == "split":
            recs = [record(L, lambda st: step.enqueue_main(st, True), stream), record(L, step.enqueue_txt_bwd, stream)]
        elif how == "dp":
            from etpnav_amd import dp
            groups = dp.planner_buckets_layered(model, text_groups=2)[2]
            assert len(groups) == 2
            recs = [record(L, lambda st: step.run_data_parallel(groups, lambda i, side: None, stream=st, overlapped=True), stream)]
        else:
            recs = [record(L, lambda st: step.run_eager(stream=st), stream)]
        owned, api = [], {}
        for k, p in enumerate(parts):
            o, a = planner_owned(p)
            owned += o
            api.update({(f"part{k} " if len(parts) > 1 else "") + n: t for n, t in a.items()})
        outputs = {**api, **grad_slices(model)}
        for r in recs:
            check_fidelity(r, whole_step=(how != "split"))
        if overlap is True and how == "step" and not env:
            assert recs[0].n_streams == 4 and recs[0].n_kernels > 100
        failures, n_runs, worst = run_orders(recs, stream, owned, outputs, ref, tol)
        report(case, recs, n_runs, worst)
        assert not failures, "\n".join(failures[:20])
    finally:
        torch.cuda.synchronize()
        for r in locals().get("recs", []):
            r.destroy()
        step.close()


@pytest.mark.parametrize("dtype", [torch.bfloat16])
def test_recorded_mlm_step_is_order_independent(dtype, stream):
    from oracle.make_golden_pretrain import make_case
    from etpnav_amd.pretrain import MlmStep
    L = _lib.lib()
    cfg, P, batch = make_case()
    model = GlocalTextPathNavCMT(cfg.to_dict(), dtype=dtype, device="cuda")
    model.load_state_dict(P, strict=True)
    model.eval()
    rates = (0.1, 0.1, 0.1, 0.0)

    def owned_of(st):
        eng = st.eng
        own = [st.st_txt, st.ws_txt, st.st_pano, st.ws_pano, st.st_mlm, st.ws_mlm, eng.grads] + ([eng.shadow] if eng.shadow is not None else [])
        api = {"txt": st.txt, "pano": st.pano, "pmask": st.pmask, "gimg": st.gimg, "d_txt": st.d_txt, "d_gimg": st.d_gimg,
               "d_pano": st.d_pano, "loss": st.loss}
        return own + list(api.values()), api

    one = MlmStep(model, batch, dropout=rates, drop_seed=9, overlap=False)
    owned, api = owned_of(one)
    poison(owned)
    torch.cuda.synchronize()
    one.run_eager()
    torch.cuda.synchronize()
    ref = snapshot({**api, **grad_slices(model)})
    one.close()
    assert not any(bool(t.isnan().any()) for n, t in ref.items() if n.startswith("grad ") or n == "loss")
    step = MlmStep(model, batch, dropout=rates, drop_seed=9, overlap=True)
    rec = None
    try:
        step.step_no = -1
        step.run_eager()
        torch.cuda.synchronize()
        rec = record(L, lambda st: step.run_eager(), stream)          # MlmStep issues on torch's current stream: a name like any other
        check_fidelity(rec, whole_step=True)
        assert rec.n_streams == 3
        owned, api = owned_of(step)
        failures, n_runs, worst = run_orders([rec], stream, owned, {**api, **grad_slices(model)}, ref, 2e-3)
        report("mlm_pretrain", [rec], n_runs, worst)
        assert not failures, "\n".join(failures[:20])
    finally:
        torch.cuda.synchronize()
        if rec is not None:
            rec.destroy()
        step.close()


# ---- the checker's own sensitivity on the GPU: two under-synchronised toy programs and their joined twins ---------------------------------
N_TOY = 1 << 12


def _toy(kind, joined):
    """-> (program(stream), owned tensors, outputs).  Built from the thin entry points only."""
    L = _lib.lib()
    dev = "cuda"
    a = torch.full((N_TOY,), 3.0, device=dev)
    b = torch.full((N_TOY,), 5.0, device=dev)
    x, y = torch.empty(N_TOY, device=dev), torch.empty(N_TOY, device=dev)
    z = torch.empty(N_TOY, dtype=torch.uint8, device=dev)
    side = ctypes.c_void_p()
    check(L.etp_stream_create(ctypes.byref(side)), "stream_create")
    s1 = side.value
    copy = lambda src, dst, s: check(L.etp_copy_f32(ptr(src), ptr(dst), N_TOY, s), "copy_f32")
    after = lambda f, t: check(L.etp_stream_after(f, t), "stream_after")

    def consumer_forked_before_its_producer(s0):
        check(L.etp_memset_async(ptr(z), 0xA5, N_TOY, s0), "memset")
        if not joined:
            after(s0, s1)                        # too early: the producer is not enqueued yet
        copy(a, x, s0)                           # producer of x
        if joined:
            after(s0, s1)
        copy(x, y, s1)                           # consumer of x
        after(s1, s0)

    def overwriter_forked_before_a_reader(s0):
        check(L.etp_memset_async(ptr(z), 0xA5, N_TOY, s0), "memset")
        copy(a, x, s0)
        after(s0, s1)
        copy(x, y, s1)                           # reader of x
        if joined:
            after(s1, s0)
        copy(b, x, s0)                           # overwrites x while the reader may still be due
        after(s1, s0)

    fn = consumer_forked_before_its_producer if kind == "consumer" else overwriter_forked_before_a_reader
    return fn, s1, [x, y, z], {"x": x, "y": y, "z": z}


@pytest.mark.parametrize("kind", ["consumer", "overwriter"])
def test_checker_flags_under_synchronised_toy_programs(kind, stream):
    L = _lib.lib()
    verdict = {}
    for joined in (True, False):
        fn, s1, owned, outputs = _toy(kind, joined)
        rec = record(L, fn, stream)              # recorded only: nothing of these programs is ever issued eagerly
        try:
            assert rec.n == (3 if kind == "consumer" else 4) and rec.n_streams == 2
            check_fidelity(rec, whole_step=True)
            # the reference: the program's own issue order as one chain
            chain = rec.chain(list(range(rec.n)))
            poison(owned)
            torch.cuda.synchronize()
            chain.launch(stream)
            check(L.etp_stream_sync(stream), "stream_sync")
            chain.destroy()
            ref = snapshot(outputs)
            assert float(ref["y"][0]) == 3.0 and float(ref["x"][0]) == (3.0 if kind == "consumer" else 5.0)
            failures, n_runs, _ = run_orders([rec], stream, owned, outputs, ref, 1e-4)
            assert n_runs == 2
            verdict[joined] = failures
        finally:
            rec.destroy()
            torch.cuda.synchronize()
            L.etp_stream_destroy(s1)
    assert verdict[True] == [], verdict[True]
    assert verdict[False], f"the under-synchronised {kind} program passed every order"
    assert any(f.startswith("[late stream") and " y:" in f for f in verdict[False]), verdict[False]


def test_linearize_refuses_what_is_not_a_permutation(stream):
    L = _lib.lib()
    fn, s1, _owned, _outputs = _toy("overwriter", True)
    rec = record(L, fn, stream)
    try:
        assert rec.n == 4
        g = ctypes.c_void_p()
        for order in ([0, 1, 2], [0, 1, 2, 2], [0, 1, 2, 4], [0, 1, 2, 3, 3]):
            arr = (ctypes.c_int32 * len(order))(*order)
            assert L.etp_graph_linearize(rec.h, arr, len(order), ctypes.byref(g)) == -1      # ETP_ERR_INVALID
        assert [rec.name(i) for i in range(rec.n)][0] == "memset" and "copy_f32" in rec.name(1)
        chain = rec.chain([0, 1, 2, 3])
        assert sr.graph_closure(chain.n, chain.edges) == [0, 1, 3, 7]
        chain.destroy()
    finally:
        rec.destroy()
        L.etp_stream_destroy(s1)
