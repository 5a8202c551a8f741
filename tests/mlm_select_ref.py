"""numpy restatement of the MLM task's masked-row selection (etp_mlm_select, csrc/traj_batch.hip): from the flat int32 labels of a batch
(-1 = not masked) the row gather etp_mlm_fwd reads, the transposed CSR pointer etp_mlm_bwd reads and the gathered labels -- what
MlmStep's host route builds with torch.nonzero and cumsum.  tests/test_mlm_select_ref_cpu.py pins it bit for bit to those statements;
tests/test_mlm_select_gpu.py compares the kernel with it.  Also the memory-safety predicate the header states for ANY content of
txt_labels, as a function both files use."""
import numpy as np

ERR_COUNT, ERR_LABEL = 1, 2
VOCAB = 30528                    # the pre-training vocabulary (run_pt/r2r_model_config_dep.json), padded as the MLM head has it


def select(txt_labels, mutate=None):
    """txt_labels: int array of any shape -> (rows int32 [Nm], ptr_t int32 [n + 1], labels int64 [Nm], count)
    `mutate` plants one wrong reading (the CPU file shows that each is rejected)."""
    lab = np.asarray(txt_labels).reshape(-1)
    n = lab.shape[0]
    rows = np.asarray([i for i in range(n) if lab[i] != -1], dtype=np.int32)
    ptr_t = np.zeros(n + 1, dtype=np.int32)
    for i in range(n):
        ptr_t[i + 1] = ptr_t[i] + (1 if lab[i] != -1 else 0)
    labels = np.asarray([lab[i] for i in rows], dtype=np.int64)
    if mutate == "rows_off_by_one":
        rows = rows + 1
    elif mutate == "ptr_inclusive":
        ptr_t = np.concatenate([ptr_t[1:], ptr_t[-1:]])
    elif mutate == "descending":
        rows, labels = rows[::-1].copy(), labels[::-1].copy()
    elif mutate == "labels_at_rows_plus_1":
        labels = np.asarray([lab[min(i + 1, n - 1)] for i in rows], dtype=np.int64)
    elif mutate == "count_left_out":
        ptr_t[n] = 0
    else:
        assert mutate is None, mutate
    return rows, ptr_t, labels, int(len(rows))


MUTATIONS = ("rows_off_by_one", "ptr_inclusive", "descending", "labels_at_rows_plus_1", "count_left_out")


def flags(txt_labels, vocab, n_expected):
    lab = np.asarray(txt_labels).reshape(-1)
    count = int((lab != -1).sum())
    return (ERR_COUNT if count != n_expected else 0) | (ERR_LABEL if bool(((lab < -1) | (lab >= vocab)).any()) else 0)


def safe(rows, ptr_t, labels, n, vocab, n_expected):
    """the memory-safety predicate of include/etpnav_hip.h: whatever txt_labels held, the first n_expected rows lie in [0, n) and labels
    in [0, vocab), ptr_t is non-decreasing from 0 with ptr_t[n] <= n_expected.  -> None, or what is violated."""
    rows, ptr_t, labels = np.asarray(rows), np.asarray(ptr_t), np.asarray(labels)
    if rows.shape[0] < n_expected or labels.shape[0] < n_expected or ptr_t.shape[0] < n + 1:
        return "an array is shorter than the step reads"
    r, l, p = rows[:n_expected], labels[:n_expected], ptr_t[:n + 1].astype(np.int64)
    if r.size and (r.min() < 0 or r.max() >= n):
        return f"a row outside [0, {n})"
    if l.size and (l.min() < 0 or l.max() >= vocab):
        return f"a label outside [0, {vocab})"
    if p[0] < 0 or bool((np.diff(p) < 0).any()):
        return "ptr_t decreases or starts below 0"
    if p[n] > n_expected:
        return f"ptr_t[n] = {int(p[n])} exceeds n_expected = {n_expected}"
    return None


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("first", "last", "all", "every7", "empty_row", "random15")


def pattern(name, n, vocab=VOCAB, seed=0):
    """flat int32 labels of length n.  'empty_row': two adjacent rows (halves) of which the second is empty; 'random15': 15 % masked
    with the labels 0 and vocab - 1 both present when at least two are masked."""
    rng = np.random.default_rng(seed * 1000003 + n)
    lab = np.full(n, -1, dtype=np.int32)
    tok = lambda k: rng.integers(0, vocab, size=k, dtype=np.int64).astype(np.int32)
    if name == "first":
        lab[0] = tok(1)[0]
    elif name == "last":
        lab[n - 1] = tok(1)[0]
    elif name == "all":
        lab[:] = tok(n)
    elif name == "every7":
        lab[::7] = tok(len(lab[::7]))
    elif name == "empty_row":
        half = max(1, n // 2)
        lab[:half:2] = tok(len(lab[:half:2]))
    elif name == "random15":
        m = rng.random(n) < 0.15
        if not m.any():
            m[rng.integers(n)] = True
        lab[m] = tok(int(m.sum()))
        idx = np.nonzero(m)[0]
        if len(idx) >= 2:
            lab[idx[0]], lab[idx[-1]] = vocab - 1, 0
    else:
        raise KeyError(name)
    return lab
