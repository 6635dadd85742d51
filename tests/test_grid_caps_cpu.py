"""tests/grid_caps.py on the CPU: the cap table agrees with the launch code's text, every case built for
tests/test_gpu_grid_caps.py is past its threshold with its witnesses inside the second trip, and the restatements the
GPU tests compare with agree with plainer ones at a small size."""
import math

import numpy as np
import pytest
import torch

import grid_caps as G


# ---------------------------------------------------------------------------------------------------------------------
# the table against the source text
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.CAPS))
def test_cap_constants_in_the_source_match_the_table(name):
    """A changed cap (or a rewritten launch line) fails here: the GPU test's sizes are derived from this table."""
    c = G.CAPS[name]
    found = G.source_caps(name)
    assert len(found) == c.hits, f"{c.file}: {len(found)} launch sites match, the table expects {c.hits}"
    for groups in found:
        if c.cap is None:
            assert groups == ()
        else:
            assert groups and all(v == c.cap for v in groups), (name, groups, c.cap)


def test_every_kernel_of_the_table_exists_in_its_file():
    for name, c in G.CAPS.items():
        text = open(G.os.path.join(G.CSRC, c.file)).read()
        for k in c.kernels:
            assert f" {k}(" in text or f" {k}<" in text, (name, k)


def test_thresholds():
    want = {"validate": 524_288, "shard": 2_097_152, "uniq": 2_097_152, "gather_rows": 32_768, "spread": 16_777_216,
            "pna_long": 262_144, "long_rows": 524_288, "hub_chunks": 1024, "char": 16_777_216, "max_degree": 262_144,
            "pack": 1_048_576, "zero_rowptr": 262_144, "hub_list": 524_288, "gru_gates_backward": 16_777_216}
    for name, thr in want.items():
        assert G.threshold(name) == thr, name
    rows = {64: 32_768, 48: 32_768, 128: 16_384, 256: 8192, 512: 8192, 50: 8192, 300: 8192, 130: 8192, 301: 8192}
    for dim, thr in rows.items():
        assert G.threshold("row_epilogue_backward", G.row_epilogue_rows_per_wg(dim)) == thr, dim


def test_row_epilogue_shapes_cover_every_route_and_the_unlaunched_scalar_one():
    routes = {G.row_epilogue_route(d) for _, d in G.ROW_EPILOGUE_SHAPES}
    assert routes == {(4, 16, 1), (4, 32, 1), (4, 64, 1), (4, 64, 2), (1, 64, 1), (1, 64, 4), (1, 64, 8)}
    assert G.row_epilogue_route(130) == (1, 64, 4) and G.row_epilogue_route(301) == (1, 64, 8)
    # the routes no other test launches: widths off four above 64
    for d in (64, 128, 48, 50, 256, 512, 300, 4):
        assert G.row_epilogue_route(d) not in ((1, 64, 4), (1, 64, 8))


# ---------------------------------------------------------------------------------------------------------------------
# every case is past its threshold, its witnesses lie in the second trip
# ---------------------------------------------------------------------------------------------------------------------
def _past(case, thr, ragged=True):
    assert case["size"] > thr, (case["size"], thr)
    w = case["witness"]
    assert w and all(thr <= p < case["size"] for p in w), (w, thr, case["size"])
    assert case["size"] - 1 in w, "the last element is a witness"
    if ragged:
        assert case["size"] % case["per_wg"] != 0, "the last workgroup of the second trip is only partly filled"


def test_validate_case():
    c = G.validate_case()
    _past(c, G.threshold("validate"))
    assert G.threshold("validate") in c["witness"]
    assert G.count_bad(c["bad"], c["num_nodes"]) == 3 and G.count_bad(c["clean"], c["num_nodes"]) == 0
    assert G.count_bad(c["bad"][: G.threshold("validate")], c["num_nodes"]) == 0, "a bad id in the first trip"
    vals = sorted(int(c["bad"][p]) for p in c["witness"])
    assert vals[0] < 0 and vals[1] == c["num_nodes"] and vals[2] > c["num_nodes"]


def test_shard_case():
    c = G.shard_case()
    thr = G.threshold("shard")
    _past(c, thr)
    src, dst = c["adj"][0]
    lo, hi = c["ranges"][c["rank"]]
    assert bool(((dst >= lo) & (dst < hi)).all()), "every edge ends in the rank's range: one table holds them all"
    owner = torch.bucketize(src, torch.tensor([r[1] for r in c["ranges"]]), right=True)
    assert set(owner.tolist()) == {0, 1, 2}
    for pos, wid in zip(c["witness"], c["witness_ids"]):
        assert int(src[pos]) == wid and not (lo <= wid < hi)
        assert torch.nonzero(src == wid).flatten().tolist() == [pos], "the witness id occurs once, in the second trip"
    assert c["witness"][0] == thr


def test_unique_case():
    c = G.unique_case()
    thr = G.threshold("uniq")
    _past(c, thr)
    assert [int(a[0].shape[0]) for a in c["adj"]] == [1_500_000, 700_000] and c["num_nodes"] == 70_001
    perm, rows = G.csr_order(c["adj"], c["num_nodes"])
    src = np.concatenate([s.numpy() for s, _ in c["adj"]])
    typ = np.r_[np.zeros(1_500_000, np.int64), np.ones(700_000, np.int64)]
    for slot, (t, s) in zip(c["witness"], c["witness_pairs"]):
        assert typ[perm[slot]] == t and src[perm[slot]] == s
        assert int(((typ == t) & (src == s)).sum()) == 1, "the pair occurs on one edge only"
    assert rows[c["witness"][0] - 1] != rows[c["witness"][0]], "the first witness opens a row"


def test_gather_rows_case():
    c = G.gather_rows_case()
    _past(c, G.threshold("gather_rows"))
    assert c["size"] == 32_768 + 3 and int(c["idx"][c["size"] - 3]) == c["table_rows"] - 1 and int(c["idx"][-1]) == 0
    assert 0 <= int(c["idx"].min()) and int(c["idx"].max()) < c["table_rows"]


def test_spread_shapes():
    thr = G.threshold("spread")
    for dim, slots in G.SPREAD_SHAPES.items():
        items = G.spread_items(dim, slots)
        assert items > thr and G.spread_items(dim, slots - 1) <= thr, "the smallest slot count past the threshold"
        assert dim not in (64, 128, 256), "those widths take k_segment_spread_rows"
    assert G.spread_items(3, G.SPREAD_SHAPES[3]) == 3 * 5_592_406 and G.spread_items(260, 258_112) == 65 * 258_112


def test_spread_case_small_dim():
    c = G.spread_case(3)
    _past(c, G.threshold("spread"))
    arg, rows = c["arg"].numpy(), c["rows"]
    deg = np.bincount(rows, minlength=c["num_nodes"])
    rowptr = np.r_[0, np.cumsum(deg)]
    live = deg > 0
    assert ((arg[live] >= rowptr[:-1][live, None]) & (arg[live] < rowptr[1:][live, None])).all()
    assert (arg[~live] == -1).all()
    # the items of the second trip belong to the last slot, whose row names it as the winner
    last = c["slots"] - 1
    assert c["witness"][0] // 3 == last and (arg[rows[last]] == last).all()


@pytest.mark.parametrize("rows,dim", G.ROW_EPILOGUE_SHAPES)
def test_row_epilogue_cases(rows, dim):
    per = G.row_epilogue_rows_per_wg(dim)
    thr = G.threshold("row_epilogue_backward", per)
    assert thr < rows and rows % per != 0 and rows - thr < 32, "just past the threshold, ragged"
    size = dict(size=rows, per_wg=per, witness=[thr, rows - 1])
    _past(size, thr)


def test_pna_case():
    c = G.pna_case(4)
    thr = G.threshold("pna_long")
    _past(c, thr)
    assert c["num_nodes"] == thr + 300
    deg = torch.bincount(c["targets"], minlength=c["num_nodes"])
    for r, d in c["long_rows"].items():
        assert int(deg[r]) >= d > 256
    assert {5, thr, c["num_nodes"] - 1} <= set(c["long_rows"]) and {257, 300} == set(c["long_rows"].values())
    assert int((deg > 256).sum()) == len(c["long_rows"])
    assert torch.equal(c["live"][c["compact"]], c["targets"]) and int((deg > 0).sum()) == c["live"].shape[0]
    assert not bool((c["targets"][1:] >= c["targets"][:-1]).all()), "message order is not CSR order"


def test_hub_case():
    c = G.hub_case()
    thr = G.threshold("hub_chunks")
    _past(c, thr, ragged=False)
    E = int(c["deg"].sum())
    assert 2048 < E < (1 << 21), "below the side streams' threshold: the hub launch runs on the caller's stream"
    assert int(c["deg"][c["hub_row"]]) == 1_100_000 and int((c["deg"] > 2048).sum()) == 1
    assert len(c["entries"]) > thr and all(r == c["hub_row"] for _, r in c["entries"])
    assert torch.equal(torch.bincount(c["adj"][0][1], minlength=c["num_nodes"]), c["deg"])


def test_side_stream_case():
    c = G.side_stream_case()
    thr = G.threshold("long_rows")
    _past(c, thr)
    E = int(c["deg"].sum())
    assert (1 << 21) <= E < (1 << 22), "the side-stream route, and the plan build's one-level form"
    assert c["num_nodes"] == thr + 600
    assert all(256 < d <= 2048 for d in c["long_rows"].values())
    assert any(r < thr for r in c["long_rows"]) and thr in c["long_rows"] and c["num_nodes"] - 1 in c["long_rows"]
    assert c["hub_size"] > G.threshold("hub_chunks") and all(p >= G.threshold("hub_chunks") for p in c["hub_witness"])
    assert int(c["deg"].argmax()) == c["max_degree_row"] >= G.threshold("max_degree")
    assert int(c["deg"].max()) == 1_200_000
    assert torch.equal(torch.bincount(c["adj"][0][1], minlength=c["num_nodes"]), c["deg"])
    # exact integer sums: |message| <= 4, so every partial sum of a row stays below 2^24
    assert 4 * int(c["deg"].max()) < (1 << 24)


def test_char_cases():
    thr = G.threshold("char")
    c = G.char_embed_case()
    _past(c, thr)
    q = c["dim"] // 4
    assert c["dim"] % 4 == 0 and c["dim"] <= 1024 and c["W"] <= 16 and c["size"] == c["B"] * c["R"] * q
    assert (c["B"] - 2) * c["R"] * q <= thr, "no sample to spare"
    c = G.window_max_case()
    _past(c, thr)
    assert c["dim"] % 4 != 0 and c["size"] == c["B"] * c["dim"] and (c["B"] - 6) * c["dim"] <= thr
    c = G.window_max_backward_case()
    _past(c, thr)
    assert c["size"] == c["B"] * c["R"] * c["dim"] and (c["B"] - 4) * c["R"] * c["dim"] <= thr
    assert int(c["arg"].min()) == 0 and int(c["arg"].max()) == c["R"] - 1


def test_plan_build_cases():
    c = G.pack_case()
    _past(c, G.threshold("pack"))
    assert len(c["adj"]) == 65 and sum(int(a[0].shape[0]) for a in c["adj"][:64]) == c["size"]
    c = G.zero_rowptr_case()
    _past(c, G.threshold("zero_rowptr"))
    c = G.hub_list_case()
    _past(c, G.threshold("hub_list"))
    assert sorted({r for _, r in c["entries"]}) == [7, G.threshold("hub_list"), c["num_segments"] - 1]
    assert bool((c["index"][1:] >= c["index"][:-1]).all())


# ---------------------------------------------------------------------------------------------------------------------
# the restatements against plainer ones at a small size
# ---------------------------------------------------------------------------------------------------------------------
def test_count_bad_is_a_loop():
    ids = torch.tensor([0, 5, -1, 9, 10, 11, 3, -7])
    assert G.count_bad(ids, 10) == sum(1 for v in ids.tolist() if v < 0 or v >= 10) == 4


def test_csr_order_and_unique_ref_equal_a_per_edge_loop():
    g = torch.Generator().manual_seed(0)
    n, counts = 23, [60, 0, 41]
    adj = [(torch.randint(0, 9, (c,), generator=g), torch.randint(0, n, (c,), generator=g)) for c in counts]
    perm, rows = G.csr_order(adj, n)
    edges = [(int(d), t, i, int(s)) for t, (ss, dd) in enumerate(adj) for i, (s, d) in enumerate(zip(ss, dd))]
    order = sorted(range(len(edges)), key=lambda e: (edges[e][0], e))      # by destination, then type-major position
    assert perm.tolist() == order and rows.tolist() == [edges[e][0] for e in order]
    type_bits = 2
    col = [(edges[e][3] << type_bits) | edges[e][1] for e in order]
    want, slot_row, cnt = G.unique_ref(adj, n, type_bits, col)
    pairs = sorted({(t, s) for _, t, _, s in edges})
    assert [w.tolist() for w in want] == [[s for t, s in pairs if t == k] for k in range(3)]
    assert slot_row.tolist() == [pairs.index((edges[e][1], edges[e][3])) for e in order]
    assert cnt.tolist() == [len(w) for w in want] + [len(pairs)]
    p2, r2, c2 = G.plan_ref(adj, type_bits)
    assert p2.tolist() == order and c2.tolist() == col and r2.tolist() == rows.tolist()


def test_spread_ref_equals_a_per_slot_loop():
    g = torch.Generator().manual_seed(1)
    n, E, D = 7, 40, 3
    dst = torch.randint(0, n, (E,), generator=g)
    perm, rows = G.csr_order([(dst, dst)], n)
    grad = torch.randn(n, D, generator=g).numpy()
    arg = torch.randint(0, E, (n, D), generator=g).numpy().astype(np.int32)
    for a in (None, arg):
        want = np.full((E, D), np.nan, dtype=np.float32)
        for s in range(E):
            for c in range(D):
                want[perm[s], c] = grad[rows[s], c] if a is None or a[rows[s], c] == s else 0.0
        np.testing.assert_array_equal(G.spread_ref(grad, a, perm, rows), want)


@pytest.mark.parametrize("flags", sorted(G.ROW_EPILOGUE_FLAGS))
def test_row_epilogue_autograd_equals_the_written_out_formulas(flags):
    c = G.row_epilogue_case(37, 10, flags)
    got = G.row_epilogue_ref(c["x"], c["gy"], c["gamma"], c["beta"], flags, torch.float64)
    want = G.row_epilogue_plain(c["x"], c["gy"], c["gamma"], c["beta"], flags)
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_allclose(a.numpy(), b, rtol=0, atol=1e-12)


def test_segment_ref64_and_small_int_messages():
    m = G.small_int_messages(500, 4, seed=2)
    assert bool((m == m.round()).all()) and float(m.abs().max()) <= 4 and bool((m[:, 0] == 1).all())
    assert float(m[:, 1:3].max()) == 3.0 and float(m[:, 3].max()) == 4.0
    dst = torch.randint(0, 9, (500,), generator=torch.Generator().manual_seed(3))
    s = G.segment_ref64(m, dst, 11, "sum")
    for r in range(11):
        assert torch.equal(s[r], m[dst == r].double().sum(0))
    mean = G.segment_ref64(m, dst, 11, "mean")
    assert torch.equal(mean[9], torch.zeros(4, dtype=torch.float64)) and float(mean[0, 0]) == 1.0
    assert G.hub_entries_of([3, 2049, 0, 5000]) == [(0, 1), (1, 1), (2, 1)] + [(c, 3) for c in range(2, 7)]


def test_char_restatements():
    from char_embedder_cases import _conv
    g = torch.Generator().manual_seed(4)
    C, L, W, F, B = 5, 6, 2, 8, 3
    chars = torch.randint(0, C, (B, L), generator=g)
    w1, b1 = torch.randn(F, C, W, generator=g).double(), torch.randn(F, generator=g).double()
    table = G.char_table(w1)
    a1 = torch.relu(_conv(torch.eye(C, dtype=torch.float64)[chars], w1, b1))            # [B, R, F]
    for b in range(B):
        for p in range(L - W + 1):
            row = b1 + sum(table[k * C + int(chars[b, p + k])] for k in range(W))
            assert float((torch.relu(row) - a1[b, p]).abs().max()) <= 1e-12
    x = torch.randint(-2, 3, (B * 4, F), generator=g).float()
    best, first = G.window_max_ref(x, B, 4, 3)
    for b in range(B):
        for d in range(F):
            col = x[b * 4: b * 4 + 3, d].tolist()
            assert float(best[b, d]) == max(col) and int(first[b, d]) == col.index(max(col))
    grad, arg = torch.randn(B, F, generator=g), torch.randint(0, 4, (B, F), generator=g).to(torch.int32)
    gx = G.window_max_backward_ref(grad, arg, 4).reshape(B, 4, F)
    for b in range(B):
        for d in range(F):
            for p in range(4):
                assert float(gx[b, p, d]) == (float(grad[b, d]) if int(arg[b, d]) == p else 0.0)
    assert math.isfinite(float(gx.sum()))
