"""Single decoding steps for the kernels of csrc/decode_step.hip and csrc/beam_step.hip whose decisions rest on EXACT ties and
on the edge rows of the radix select (csrc/decode_common.h): the generators, and the input condition under which the float32
kernel must reproduce the restatements of tests/greedy_cases.py (dict_step, through test_gpu_greedy.restated_step) and
tests/beam_cases.py (restated_crafted_step).  CPU only; tests/test_decode_ties_cpu.py checks every case here,
tests/test_gpu_decode_ties.py runs them.

The grid.  Every sum score + bias is a multiple of GRID = 1/8 of magnitude below 2^12 (the shared-key-byte rows: of 2^-9
below 2^15, without a bias or under one of zeros), and the bias is on the same grid or absent, so the sum is exact in
float32.  Equal sums then give bit-equal log-probabilities inside the kernel ((v - max) - log sum) and inside the float32
and float64 restatements (v - norm); parents of one sample that share a row, the copy scores and the slot score give
bit-equal candidates.  Slots that do not share their score are SLOT = 0.5625 apart: an odd multiple of GRID / 2, so that
plain entries of different parents never coincide.

The input condition (`hold`) replaces `gap >= MARGIN` of the tie-free tests.  Of every chosen candidate and every other
candidate of the sample, and of the vocabulary score of every group id and the values at the K-th / (K+1)-th and W-th /
(W+1)-th places of its row, the two values are either exactly equal in float64 AND in float32, or at least MARGIN apart in
float64; and the float32 and float64 restatements choose the same (parent, class, id) lists, all at finite scores.  Seeds
are searched as beam_cases.crafted_with_margin does.

Rows with -inf columns keep the top-1 finite, and slot 0 of every beam sample has a finite score: a parent at -inf writes
the ids 0 .. W - 1 in the kernel where the restatement lists the W best ids of its row.  The two can only be told apart
when a candidate at -inf is chosen, that is when every slot of the sample is at -inf, which decoding cannot reach (slot 0
starts at 0 and a sample always has W finite candidates).  NaN scores are not defined by the restatement and not used."""
import math

import numpy as np
import torch

from beam_cases import restated_crafted_step, select, slot_entries
from greedy_cases import MARGIN

INF = math.inf
GRID = 0.125
SLOT = 0.5625
BLOCK = 1024                 # kDecThreads: the columns of one step of the tie scan
ATTEMPTS = 8


# ---------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------
def tie_row(V, n, run, need, gen, flat, t=0.0, masked=0):
    """Sums [V] (float64, on the grid) whose n-th largest value t is held by the columns `run`, `need` of them among the n
    largest: n - need other columns are larger (`flat`: one at t + 2 GRID, the others at t + GRID; else t + GRID, t + 2 GRID,
    ... all distinct), the rest lower by 8 .. 63 GRID, one of them (`out`) by GRID alone.  The last `masked` of the lower
    columns are -inf.  -> (row, the top-1 column, `out` or None)."""
    run = sorted(run)
    held = set(run)
    others = [c for c in range(V) if c not in held]
    others = [others[i] for i in torch.randperm(len(others), generator=gen).tolist()]
    larger, lower = others[:n - need], others[n - need:]
    assert 1 <= need <= len(run) and len(larger) == n - need
    row = torch.full((V,), float(t), dtype=torch.float64)
    if larger:
        step = torch.ones(len(larger), dtype=torch.float64) if flat else 1.0 + torch.arange(len(larger), dtype=torch.float64)
        row[larger] = t + GRID * step
        if flat:
            row[larger[0]] = t + 2 * GRID
    if lower:
        row[lower] = t - GRID * torch.randint(8, 64, (len(lower),), generator=gen).double()
        row[lower[0]] = t - GRID
        if masked:
            row[lower[len(lower) - masked:]] = -INF
    top1 = int(torch.sort(row, descending=True, stable=True).indices[0])
    out = lower[0] if lower and masked < len(lower) else None
    return row, top1, out


def probe(row, top1, column):
    """Two copy scores whose group on `column` decides the prediction by its admission to the top K: merged with the
    column's vocabulary entry it beats the row's top-1, on its own it loses.  Close rows (the column within 0.5 of the
    top-1): the group is 0.3 below the top-1, as in test_a_merge_inside_the_top_k_overturns_the_top_1_and_outside_it_does_
    not (so is a group on a column so far down, -inf included, that merging cannot lift it).  Else, with a = exp(column -
    top-1), the group is at log(1 - a / 2): merged log(1 + a / 2) above, alone as far below."""
    d = float(row[top1] - row[column])
    a = math.exp(-d)
    group = float(row[top1]) + (-0.3 if d <= 0.5 or a < 4 * MARGIN else math.log1p(-a / 2.0))
    return [group - math.log(2.0)] * 2


def place_of(row, n):
    """What a row holds at its n-th place: (the columns of the tie run, how many of them are among the n largest, the
    last of those = the kernel's cut)."""
    row = np.asarray(row, dtype=np.float64)
    kth = np.sort(row)[::-1][n - 1]
    run = np.nonzero(row == kth)[0].tolist()
    need = n - int((row > kth).sum())
    return run, need, run[need - 1]


# ---------------------------------------------------------------------------------------------------------------------
# assembling a step
# ---------------------------------------------------------------------------------------------------------------------
def grid_bias(V, gen):
    return GRID * torch.randint(-16, 17, (V,), generator=gen).double()


def assemble(samples, bias, gen, W=None):
    """samples: dicts with rows (one [V] float64 row of sums, or W of them), groups [(id, [copy scores])] and, for the
    beam, slots [W] -> the inputs of test_gpu_greedy.run_step (W None) or test_gpu_beam.run_step, the memories shuffled.
    The copy scores of a memory are the same for every parent."""
    rows = torch.stack([r for s in samples for r in s["rows"]])
    scores = (rows - bias if bias is not None else rows).float()
    index, ids, copy = [], [], []
    for b, s in enumerate(samples):
        for g, values in s.get("groups", []):
            index += [b] * len(values)
            ids += [g] * len(values)
            copy += values
    index, ids = torch.tensor(index, dtype=torch.int64), torch.tensor(ids, dtype=torch.int64)
    copy = torch.tensor(copy, dtype=torch.float64).float()
    shuffle = torch.randperm(index.shape[0], generator=gen)
    index, ids, copy = index[shuffle], ids[shuffle], copy[shuffle]
    bias = bias.float() if bias is not None else None
    if W is None:
        return scores, bias, copy, index, ids, torch.zeros(len(samples), dtype=torch.bool)
    beam = torch.tensor([s["slots"] for s in samples], dtype=torch.float32)
    done = torch.zeros(len(samples), W, dtype=torch.bool)
    return scores, bias, copy.unsqueeze(1).repeat(1, W).contiguous(), index, ids, beam, done


def sums_of(inputs):
    """score + bias of a step's inputs in float32, as the kernel adds them."""
    scores, bias = inputs[0], inputs[1]
    return scores + bias if bias is not None else scores + 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the input condition
# ---------------------------------------------------------------------------------------------------------------------
def log_rows(inputs, W, dtype):
    """([B, W, V] vocabulary, [I, W] copy) log-probabilities of a step's inputs in `dtype`: the joint normaliser of
    test_gpu_greedy.restated_step / beam_cases.restated_crafted_step."""
    scores, bias, copy, index = inputs[:4]
    B = scores.shape[0] // W
    s = (scores.to(dtype) + (bias.to(dtype) if bias is not None else 0)).reshape(B, W, -1)
    c = copy.to(dtype).reshape(-1, W)
    total = torch.full((B, W), -INF, dtype=dtype)
    for b in range(B):
        if bool((index == b).any()):
            total[b] = torch.logsumexp(c[index == b], 0)
    norm = torch.logaddexp(torch.logsumexp(s, -1), total)
    return (s - norm.unsqueeze(-1)).numpy(), (c - norm[index]).numpy()


def pools_of(inputs, top_k, W, dtype):
    """Per sample {(parent, id): (score, class)}: the candidates beam_cases.beam_step ranks (greedy: W = 1, slot score 0)."""
    index, ids = inputs[3].numpy(), inputs[4].numpy()
    rows, copies = log_rows(inputs, W, dtype)
    B = rows.shape[0]
    slots = inputs[5].numpy().astype(rows.dtype) if len(inputs) == 7 else np.zeros((B, 1), dtype=rows.dtype)
    pools = []
    for b in range(B):
        mine = np.nonzero(index == b)[0]
        pool = {}
        for j in range(W):
            entries, best, _ = slot_entries(rows[b, j], copies[mine, j], ids[mine], top_k, W)
            for g, value in entries.items():
                pool[(j, g)] = (slots[b, j] + value, 0 if g in best else 1)
        pools.append(pool)
    return pools, rows


def _apart_or_equal(d64, d32):
    d64, d32 = (np.where(np.isnan(d), 0.0, d) for d in (np.asarray(d64, dtype=np.float64), np.asarray(d32, dtype=np.float64)))
    return bool((((d64 == 0) & (d32 == 0)) | (np.abs(d64) >= MARGIN)).all())


def hold(inputs, top_k, W):
    """The input condition of the module docstring -> (whether it holds, per sample the (parent, class, id) lists the
    float64 restatement chooses)."""
    with np.errstate(invalid="ignore"):
        pools64, rows64 = pools_of(inputs, top_k, W, torch.float64)
        pools32, rows32 = pools_of(inputs, top_k, W, torch.float32)
        index, ids = inputs[3].numpy(), inputs[4].numpy()
        V = rows64.shape[2]
        K = min(top_k, V)
        ok, chosen = True, []
        for b, (p64, p32) in enumerate(zip(pools64, pools32)):
            keys = list(p64)
            if set(keys) != set(p32):
                return False, None
            first = [select([(v, j, cls, g) for (j, g), (v, cls) in pool.items()], W)[0] for pool in (p64, p32)]
            picks = [[(c[1], c[2], c[3]) for c in ranked] for ranked in first]
            chosen.append(picks[0])
            ok = ok and picks[0] == picks[1] and all(c[0] > -INF for c in first[0])
            v64 = np.array([float(p64[k][0]) for k in keys])
            v32 = np.array([float(p32[k][0]) for k in keys])
            for c in first[0]:
                at = keys.index((c[1], c[3]))
                ok = ok and _apart_or_equal(v64[at] - v64, v32[at] - v32)
            groups = [int(g) for g in set(ids[index == b].tolist()) if g < V]
            for j in range(W):
                if not groups or not inputs_slot_is_finite(inputs, b, j):
                    continue
                r64, r32 = rows64[b, j], rows32[b, j]
                order = np.argsort(-r64, kind="stable")
                ok = ok and np.array_equal(order[:K + 1], np.argsort(-r32, kind="stable")[:K + 1])
                places = ([K - 1, K] if K < V else []) + ([W - 1, W] if W < V else [])
                for place in places:
                    ok = ok and _apart_or_equal(r64[groups] - r64[order[place]], r32[groups] - r32[order[place]])
    return bool(ok), chosen


def inputs_slot_is_finite(inputs, b, j):
    return len(inputs) != 7 or float(inputs[5][b, j]) > -INF


# ---------------------------------------------------------------------------------------------------------------------
# greedy cases: name -> builder(seed) -> (inputs, top_k, per-sample notes)
# A note: family, and where it applies n / run / need / cut (what tests/test_decode_ties_cpu.py recounts), `expect` (the
# predicted id) and `pair` (the note's sample and the next one are the two probes of one cut: inside, outside).
# ---------------------------------------------------------------------------------------------------------------------
def _probe_pair(row, top1, inside, outside, note):
    """Two samples on one row: a group on the last admitted column, a group on the first column that is not."""
    return [dict(rows=[row], groups=[(inside, probe(row, top1, inside))], note=dict(note, expect=inside, pair=True)),
            dict(rows=[row], groups=[(outside, probe(row, top1, outside))], note=dict(note, expect=top1))]


def _run_pair(V, K, run, need, gen, flat=True, family="k-run", **kw):
    run = sorted(run)
    row, top1, out = tie_row(V, K, run, need, gen, flat, **kw)
    outside = run[need] if need < len(run) else out
    note = dict(family=family, n=K, run=run, need=need, cut=run[need - 1])
    return _probe_pair(row, top1, run[need - 1], outside, note)


def _random_run(V, m, gen, lo=1, hi=None):
    hi = V - 1 if hi is None else hi
    return sorted((lo + torch.randperm(hi - lo, generator=gen)[:m]).tolist())


def greedy_small_runs(seed, V=300, K=100):
    """Family 1 inside one block: need = 1, need = m - 1, need = m (no scan), the run on column 0 and column V - 1."""
    g = torch.Generator().manual_seed(seed)
    samples = _run_pair(V, K, _random_run(V, 5, g), 1, g) + _run_pair(V, K, _random_run(V, 5, g), 4, g) \
        + _run_pair(V, K, _random_run(V, 5, g), 5, g) + _run_pair(V, K, [0] + _random_run(V, 1, g) + [V - 1], 2, g)
    return assemble(samples, grid_bias(V, g), g), K, [s["note"] for s in samples]


def greedy_blocks(seed, V=2500, K=100):
    """Family 1 across blocks: a run over three blocks with the cut in the middle one, the cut at column 1023 and at
    column 1024, and a run longer than a block (1500 of 2500 columns, 40 distinct larger ones)."""
    g = torch.Generator().manual_seed(seed)
    spread = _random_run(V, 2, g, 1, 1000) + _random_run(V, 2, g, 1100, 2000) + _random_run(V, 2, g, 2100, V - 1)
    long_run = sorted(torch.randperm(V, generator=g)[:1500].tolist())
    samples = _run_pair(V, K, spread, 3, g) + _run_pair(V, K, [5, 1023, 1024, 2047, 2048], 2, g) \
        + _run_pair(V, K, [5, 1023, 1024, 2047, 2048], 3, g) + _run_pair(V, K, long_run, K - 40, g, flat=False)
    return assemble(samples, grid_bias(V, g), g), K, [s["note"] for s in samples]


def greedy_all_equal(seed, V=1025, K=100):
    """Every column equal (the cut is column K - 1), with and without a bias."""
    g = torch.Generator().manual_seed(seed)
    samples = _run_pair(V, K, list(range(V)), K, g)
    return assemble(samples, grid_bias(V, g) if seed % 2 else None, g), K, [s["note"] for s in samples]


def greedy_v_is_k_plus_1(seed, V=101, K=100):
    g = torch.Generator().manual_seed(seed)
    samples = _run_pair(V, K, _random_run(V, 3, g, 0, V), 2, g) + _run_pair(V, K, [0, V - 1], 1, g)
    return assemble(samples, grid_bias(V, g), g), K, [s["note"] for s in samples]


def greedy_top1(seed, V=2049, K=100):
    """Family 3: the maximum held by two columns of one thread (c, c + 1024), of two lanes of a wave, of two waves, and by
    column V - 1; then the rank leg of the arg-max: a group that equals the top-1 bit for bit loses to it, and of two
    equal groups the lower id wins."""
    g = torch.Generator().manual_seed(seed)
    pairs = [(3, 40), (70, 700), (500, 1023)] if V == 1024 else [(0, 1024), (3, 40), (70, 700)] if V == 1025 \
        else [(7, 1031), (1000, 2048), (5, 2048), (3, 40), (70, 1500)]
    samples = []
    for a, b in pairs:
        row, _, _ = tie_row(V, 2, [a, b], 2, g, False)
        samples.append(dict(rows=[row], note=dict(family="top-1", n=2, run=[a, b], need=2, cut=b, expect=a)))
    row, top1, _ = tie_row(V, 2, [pairs[0][0], pairs[0][1]], 2, g, False)
    best = float(row[top1])
    samples.append(dict(rows=[row], groups=[(V + 2, [best])], note=dict(family="rank", expect=top1)))
    samples.append(dict(rows=[row], groups=[(V + 4, [best + 1.0]), (V + 2, [best + 1.0]), (7, [best - 3.0])],
                        note=dict(family="rank", expect=V + 2)))
    return assemble(samples, None, g), K, [s["note"] for s in samples]


def shared_byte_row(V, gen, kind):
    """Family 4: 16384 + i 2^-9 shuffled over the columns (keys that differ in their low 11 bits only), the same negated,
    or (i - (V - 30)) 2^-9: 29 positive columns, so that the K-th key is a flipped one."""
    i = torch.randperm(V, generator=gen).double()
    if kind == "mixed":
        return (i - (V - 30)) * 2.0 ** -9
    row = 16384.0 + i * 2.0 ** -9
    return row if kind == "positive" else -row


def greedy_shared_bytes(seed, V=2048, K=100):
    g = torch.Generator().manual_seed(seed)
    samples = []
    for kind in ("positive", "negative", "mixed"):
        row = shared_byte_row(V, g, kind)
        order = torch.sort(row, descending=True).indices.tolist()
        note = dict(family="bytes-" + kind, n=K, run=[order[K - 1]], need=1, cut=order[K - 1])
        samples += _probe_pair(row, order[0], order[K - 1], order[K], note)
    return assemble(samples, None, g), K, [s["note"] for s in samples]


def greedy_zeros(seed, V=300, K=100):
    """Family 5: the run at the K-th place is made of -0.0 sums (score -0.0 plus bias -0.0) on its first three columns and
    +0.0 sums on its last three; three fit."""
    g = torch.Generator().manual_seed(seed)
    run = _random_run(V, 6, g)
    samples = _run_pair(V, K, run, 3, g, family="zeros")
    inputs = list(assemble(samples, grid_bias(V, g), g))
    inputs[1][run] = torch.tensor([-0.0, -0.0, -0.0, -0.0, 0.0, 0.0])
    inputs[0][:, run] = torch.tensor([-0.0, -0.0, -0.0, 0.0, -0.0, 0.0])
    return tuple(inputs), K, [s["note"] for s in samples]


def greedy_masked(seed, V=300, K=100):
    """Family 6: -inf columns behind more than K, exactly K and fewer than K finite ones."""
    g = torch.Generator().manual_seed(seed)
    samples = _run_pair(V, K, _random_run(V, 5, g), 2, g, family="masked-more", masked=120)
    row, top1, _ = tie_row(V, K, _random_run(V, 3, g), 3, g, True, masked=V - K)          # exactly K finite
    masked = [c for c in range(V) if row[c] == -INF]
    run, _, cut = place_of(row, K)
    samples += _probe_pair(row, top1, cut, masked[0], dict(family="masked-exact", n=K, run=run, need=3, cut=cut))
    row, top1, _ = tie_row(V, 60, _random_run(V, 3, g), 3, g, True, masked=V - 60)        # 60 finite: the K-th is -inf
    run, need, cut = place_of(row, K)
    lowest = place_of(row, 60)[2]
    note = dict(family="masked-fewer", n=K, run=run, need=need, cut=cut)
    samples += [dict(rows=[row], groups=[(lowest, probe(row, top1, lowest))], note=dict(note, expect=lowest)),
                dict(rows=[row], groups=[(cut, probe(row, top1, cut))], note=dict(note, expect=top1)),
                dict(rows=[row], groups=[(run[need], probe(row, top1, run[need]))], note=dict(note, expect=top1))]
    return assemble(samples, grid_bias(V, g), g), K, [s["note"] for s in samples]


GREEDY = {
    "small_runs": (greedy_small_runs, 9000),
    "blocks": (greedy_blocks, 9100),
    "all_equal": (greedy_all_equal, 9200),
    "all_equal_bias": (greedy_all_equal, 9201),
    "v_is_k_plus_1": (greedy_v_is_k_plus_1, 9300),
    "top1_v1024": (lambda seed: greedy_top1(seed, 1024), 9400),
    "top1_v1025": (lambda seed: greedy_top1(seed, 1025), 9410),
    "top1_v2049": (lambda seed: greedy_top1(seed, 2049), 9420),
    "shared_bytes": (greedy_shared_bytes, 9500),
    "zeros": (greedy_zeros, 9600),
    "masked": (greedy_masked, 9700),
}


# ---------------------------------------------------------------------------------------------------------------------
# beam cases: name -> builder(seed) -> (inputs, top_k, W, per-sample notes)
# A note: family, n / run / need / cut of parent 0's row, `expect` (the chosen (parent, id) list) where the case names it,
# `pair`, and `cls`: the tie class the probed id must have in parent 0.
# ---------------------------------------------------------------------------------------------------------------------
def _slots(W, equal=False, first_step=False):
    if first_step:
        return [0.0] + [-INF] * (W - 1)
    return [-0.25 - (0.0 if equal else SLOT * j) for j in range(W)]


def _beam_pair(V, n, W, run, need, gen, family, cls, flat=True, **kw):
    run = sorted(run)
    row, top1, out = tie_row(V, n, run, need, gen, flat, **kw)
    outside = run[need] if need < len(run) else out
    note = dict(family=family, n=n, run=run, need=need, cut=run[need - 1])
    return [dict(rows=[row] * W, slots=_slots(W), groups=[(c, probe(row, top1, c))],
                 note=dict(note, probed=c, cls=k, pair=(c != outside)))
            for c, k in ((run[need - 1], cls[0]), (outside, cls[1]))]


def beam_runs(seed, V, K, W, blocks=False):
    """Families 2, 1, 7 and 8 for the beam at one (V, K, W): probes at cut_w and at cut, every parent on one row at one
    score (a unique maximum; the two best tied), rows that are permutations of one another, and the state before step 0."""
    g = torch.Generator().manual_seed(seed)

    def run_at(m):
        if blocks:                                                   # over three blocks, BLOCK - 1 and BLOCK among them
            return sorted(set(_random_run(V, 1, g, 1, 1000) + [BLOCK - 1, BLOCK] + _random_run(V, m - 3, g, 2100, V - 1)))
        return _random_run(V, m, g, 0, V)
    samples = _beam_pair(V, W, W, run_at(4), 2 if W > 2 else 1, g, "w-run", (0, 1))
    if K > W:
        samples += _beam_pair(V, K, W, run_at(4), 3 if blocks else 2, g, "k-run", (1, 1))
    row, top1, _ = tie_row(V, 1, [int(torch.randint(0, V, (1,), generator=g))], 1, g, False)
    samples.append(dict(rows=[row] * W, slots=_slots(W, equal=True),
                        note=dict(family="parents", expect=[(j, top1) for j in range(W)])))
    pair = _random_run(V, 2, g, 0, V)
    row, _, _ = tie_row(V, 2, pair, 2, g, False)
    both = [(j, c) for j in range(W) for c in pair][:W]
    samples.append(dict(rows=[row] * W, slots=_slots(W, equal=True), note=dict(family="parents", n=2, run=pair, need=2,
                                                                                cut=pair[1], expect=both)))
    run = sorted(set([0, V - 1] + run_at(3)))
    row, _, _ = tie_row(V, W, run, 1, g, False)
    rows = [row] + [row[torch.randperm(V, generator=g)] for _ in range(W - 1)]
    samples.append(dict(rows=rows, slots=_slots(W), note=dict(family="permuted", n=W, run=run, need=1, cut=0)))
    row, _, _ = tie_row(V, W, run, 2, g, False)
    samples.append(dict(rows=[row] * W, slots=_slots(W, first_step=True),
                        note=dict(family="first-step", n=W, run=run, need=2, cut=run[1])))
    return assemble(samples, grid_bias(V, g), g, W), K, W, [s["note"] for s in samples]


def beam_keys(seed, V=2048, K=100, W=3):
    """Families 4, 5 and 6 at the W-th place: shared key bytes (positive, negated, mixed signs), a run of -0.0 and +0.0
    sums (the bias is +0.0, and -0.0 under the run), and rows with more than W and with exactly W (fewer than K) finite
    columns."""
    g = torch.Generator().manual_seed(seed)
    samples = []
    for kind in ("positive", "negative", "mixed"):
        row = shared_byte_row(V, g, kind)
        order = torch.sort(row, descending=True).indices.tolist()
        samples.append(dict(rows=[row] * W, slots=_slots(W), note=dict(family="bytes-" + kind, n=W, run=[order[W - 1]], need=1,
                                                                       cut=order[W - 1])))
    zero_run = _random_run(V, 4, g, 0, V)
    row, _, _ = tie_row(V, W, zero_run, 2, g, True)
    zeros = len(samples)
    samples.append(dict(rows=[row] * W, slots=_slots(W), note=dict(family="zeros", n=W, run=zero_run, need=2, cut=zero_run[1])))
    row, _, _ = tie_row(V, W, _random_run(V, 4, g, 0, V), 2, g, True, masked=V - 40)
    run, need, cut = place_of(row, W)
    samples.append(dict(rows=[row] * W, slots=_slots(W), note=dict(family="masked-more", n=W, run=run, need=need, cut=cut)))
    row, top1, _ = tie_row(V, W, _random_run(V, 2, g, 0, V), 2, g, True, masked=V - W)
    run, need, cut = place_of(row, K)
    samples.append(dict(rows=[row] * W, slots=_slots(W), groups=[(V + 3, [float(row[top1]) - 1.0])],
                        note=dict(family="masked-fewer", n=K, run=run, need=need, cut=cut)))
    inputs = list(assemble(samples, torch.zeros(V, dtype=torch.float64), g, W))
    inputs[1][zero_run] = -0.0
    inputs[0][zeros * W:(zeros + 1) * W][:, zero_run] = torch.tensor([-0.0, 0.0, -0.0, 0.0])
    return tuple(inputs), K, W, [s["note"] for s in samples]


def beam_edges(seed, V, K, W):
    """Family 2's other runs around cut_w, without probes: all of the run fits (no scan), all but one of it, every column
    equal at equal slot scores, and past two blocks a run longer than a block and the cut at column BLOCK."""
    g = torch.Generator().manual_seed(seed)
    samples = []

    def plain(run, need, family="w-run", equal=False, **more):
        run = sorted(run)
        row, top1, _ = tie_row(V, W, run, need, g, False)
        groups = [(V + 3, [float(row[top1]) - 1.0])] if not samples else []      # one memory: the key V + 3, behind the top-1
        samples.append(dict(rows=[row] * W, slots=_slots(W, equal=equal), groups=groups,
                            note=dict(family=family, n=W, run=run, need=need, cut=run[need - 1], **more)))
    m = min(3, W)
    plain(_random_run(V, m, g, 0, V), m)
    plain(_random_run(V, 3, g, 0, V), 2)
    plain(list(range(V)), W, "all-equal", equal=True, expect=[(0, c) for c in range(W)])
    if V > 2 * BLOCK:
        plain(torch.randperm(V, generator=g)[:1500].tolist(), max(W - 3, 1), "long-run")
        plain(_random_run(V, 1, g, 1, 1000) + [BLOCK - 1, BLOCK] + _random_run(V, 1, g, 2100, V - 1), min(3, W), "cut-at-block")
    return assemble(samples, grid_bias(V, g), g, W), K, W, [s["note"] for s in samples]


BEAM = {
    "v37_k10_w3": (lambda seed: beam_runs(seed, 37, 10, 3), 9800),
    "v37_k10_w2": (lambda seed: beam_runs(seed, 37, 10, 2), 9810),
    "v37_k8_w8": (lambda seed: beam_runs(seed, 37, 8, 8), 9820),
    "v37_k3_w3": (lambda seed: beam_runs(seed, 37, 3, 3), 9830),
    "v1025_k100_w8": (lambda seed: beam_runs(seed, 1025, 100, 8), 9840),
    "v2500_k100_w8": (lambda seed: beam_runs(seed, 2500, 100, 8, blocks=True), 9850),
    "v2500_k8_w8": (lambda seed: beam_runs(seed, 2500, 8, 8, blocks=True), 9860),
    "keys_w3": (beam_keys, 9900),
    "edges_v9_k8_w8": (lambda seed: beam_edges(seed, 9, 8, 8), 9910),
    "edges_v9_k100_w8": (lambda seed: beam_edges(seed, 9, 100, 8), 9920),
    "edges_v37_k10_w2": (lambda seed: beam_edges(seed, 37, 10, 2), 9930),
    "edges_v1025_k100_w3": (lambda seed: beam_edges(seed, 1025, 100, 3), 9940),
    "edges_v2500_k100_w8": (lambda seed: beam_edges(seed, 2500, 100, 8), 9950),
    "edges_v2500_k8_w8": (lambda seed: beam_edges(seed, 2500, 8, 8), 9960),
}


# ---------------------------------------------------------------------------------------------------------------------
# seeds and expected results
# ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def build(kind, name, seed):
    """(inputs, top_k, W, notes) of one seed of a case; W = 1 for a greedy case."""
    made = (GREEDY if kind == "greedy" else BEAM)[name][0](seed)
    return (made[0], made[1], 1, made[2]) if kind == "greedy" else made


def tried(kind, name):
    """Whether the input condition holds for each of the ATTEMPTS seeds from the case's base on: computed once."""
    key = ("tried", kind, name)
    if key not in _CACHE:
        base = (GREEDY if kind == "greedy" else BEAM)[name][1]
        out = []
        for seed in range(base, base + ATTEMPTS):
            inputs, top_k, W, _ = build(kind, name, seed)
            out.append(hold(inputs, top_k, W)[0])
        _CACHE[key] = out
    return _CACHE[key]


def restated(kind, inputs, top_k, W, dtype):
    """The existing restatements, unchanged -> (greedy: dict_step's tuples per sample; beam: the chosen candidates per
    sample; the copy scores' log-sum-exp)."""
    if kind == "greedy":
        from test_gpu_greedy import restated_step
        with np.errstate(invalid="ignore"):                          # -inf - -inf in dict_step's gaps, which nothing reads
            return restated_step(*inputs[:5], top_k, dtype)
    end_id = min(3, inputs[0].shape[1] - 1)
    with np.errstate(invalid="ignore"):
        chosen, _, _, total = restated_crafted_step(*inputs, top_k, W, dtype, end_id)
    return chosen, total


def case(kind, name):
    """The case at the first seed from its base on for which the input condition holds: (inputs, top_k, W, notes, the
    float64 restatement, the float32 one, the copy scores' log-sum-exp in float32, the (parent, class, id) lists of `hold`).
    Computed once per process, shared, left unchanged."""
    key = ("case", kind, name)
    if key not in _CACHE:
        base = (GREEDY if kind == "greedy" else BEAM)[name][1]
        good = [base + i for i, ok in enumerate(tried(kind, name)) if ok]
        assert good, f"{kind} {name}: no seed in [{base}, {base + ATTEMPTS}) meets the input condition"
        inputs, top_k, W, notes = build(kind, name, good[0])
        ok, chosen = hold(inputs, top_k, W)
        assert ok
        want64, _ = restated(kind, inputs, top_k, W, torch.float64)
        want32, total = restated(kind, inputs, top_k, W, torch.float32)
        _CACHE[key] = (inputs, top_k, W, notes, want64, want32, total, chosen)
    return _CACHE[key]
