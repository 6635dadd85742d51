"""The cases of tests/tie_cases.py, checked where no GPU is needed: every case of tests/test_gpu_decode_ties.py meets the
tie-aware input condition at its seed (and at no fewer than three quarters of the seeds tried), adds score and bias
exactly, really holds the tie run, `need` and cut it is named for, and its probe pairs decide differently in the
restatement -- so that no GPU case passes vacuously."""
import numpy as np
import pytest
import torch

import tie_cases
from tie_cases import ATTEMPTS, BEAM, BLOCK, GREEDY, GRID, case, hold, place_of, sums_of, tried

CASES = [("greedy", name) for name in GREEDY] + [("beam", name) for name in BEAM]
IDS = [f"{kind}-{name}" for kind, name in CASES]


@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_at_most_a_quarter_of_the_seeds_is_rejected(kind, name):
    ok = tried(kind, name)
    assert len(ok) == ATTEMPTS and ok.count(False) * 4 <= ATTEMPTS, ok


@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_the_input_condition_holds_and_both_restatements_choose_the_same(kind, name):
    inputs, top_k, W, notes, want64, want32, _, chosen = case(kind, name)     # case() asserts hold()
    assert len(notes) == len(want64) == len(chosen) <= 8 and inputs[0].shape[1] <= 2500
    for b in range(len(notes)):
        if kind == "greedy":                                          # hold() ranks as dict_step does
            assert want64[b][0] == want32[b][0] == chosen[b][0][2]
        else:
            assert [(c[1], c[2], c[3]) for c in want64[b]] == [(c[1], c[2], c[3]) for c in want32[b]] == chosen[b]
            assert all(c[0] > -np.inf for c in want64[b])
            assert len(set((c[1], c[3]) for c in want64[b])) == W


@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_score_plus_bias_is_exact_and_on_the_grid(kind, name):
    inputs = case(kind, name)[0]
    scores, bias = inputs[0], inputs[1]
    exact = scores.double() + (bias.double() if bias is not None else 0.0)
    assert torch.equal(sums_of(inputs).double(), exact)               # the float32 sum is the real one
    finite = exact[torch.isfinite(exact)]
    fine = "bytes" in name or name == "keys_w3"
    step, bound = (2.0 ** -9, 2.0 ** 15) if fine else (GRID, 2.0 ** 12)
    assert bool((finite / step == torch.round(finite / step)).all()) and float(finite.abs().max()) < bound
    if bias is not None:
        assert bool((bias.double() / GRID == torch.round(bias.double() / GRID)).all())
    if kind == "beam":                                                # slot 0 finite: tie_cases' docstring
        assert bool(torch.isfinite(inputs[5][:, 0]).all())
    assert not bool(torch.isnan(scores).any())


@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_a_case_holds_what_it_is_named_for(kind, name):
    inputs, top_k, W, notes, want64, _, _, _ = case(kind, name)
    sums = sums_of(inputs).double().numpy()
    for b, note in enumerate(notes):
        row = sums[b * W]                                             # the sample's row (beam: parent 0's)
        if "n" in note:                                               # recount the run, `need` and the cut
            run, need, cut = place_of(row, note["n"])
            assert (run, need, cut) == (note["run"], note["need"], note["cut"]), (note["family"], b)
        if "expect" in note:
            got = want64[b][0] if kind == "greedy" else [(c[1], c[3]) for c in want64[b]]
            assert got == note["expect"], (note["family"], b)
        if note.get("pair"):                                          # this sample and the next: one cut, two decisions
            assert np.array_equal(row, sums[(b + 1) * W]) and notes[b + 1]["cut"] == note["cut"]
            if kind == "greedy":
                assert want64[b][0] == note["cut"] != want64[b + 1][0]
                continue
            picked = [[(c[1], c[2], c[3]) for c in want64[s]] for s in (b, b + 1)]
            inside, outside = note["probed"], notes[b + 1]["probed"]
            assert inside == note["cut"] and outside != inside
            assert (0, note["cls"], inside) in picked[0] and (0, 0, outside) not in picked[1]
            assert (0, 1 - note["cls"], inside) not in picked[0]
            if note["family"] == "k-run":                             # not admitted: the group alone is not chosen
                assert all(c[2] != outside for c in picked[1])
            elif top_k > W:                                           # outside cut_w, inside the top K: merged, class 1
                assert (0, 1, outside) in picked[1]
        if note["family"] == "zeros":                                 # both signs: a key that tells them apart admits others
            run, signs = note["run"], np.signbit(row[note["run"]]).tolist()
            assert bool((row[run] == 0).all()) and signs[0] and False in signs
            unfolded = [c for c, s in zip(run, signs) if not s] + [c for c, s in zip(run, signs) if s]
            assert set(unfolded[:note["need"]]) != set(run[:note["need"]])
        if note["family"].startswith("masked"):
            finite = int(np.isfinite(row).sum())
            assert np.isfinite(row.max())
            assert {"masked-more": finite > note["n"], "masked-exact": finite == note["n"],
                    "masked-fewer": finite < note["n"] and row[note["cut"]] == -np.inf}[note["family"]]


def test_the_runs_lie_where_the_tie_scan_takes_another_path():
    notes = case("greedy", "blocks")[3]
    spread, at_1023, at_1024, long_run = notes[0], notes[2], notes[4], notes[6]
    assert sorted(set(c // BLOCK for c in spread["run"])) == [0, 1, 2] and spread["cut"] // BLOCK == 1
    assert at_1023["cut"] == BLOCK - 1 and at_1024["cut"] == BLOCK
    assert len(long_run["run"]) == 1500 and long_run["need"] == 60 and long_run["n"] == 100
    small = case("greedy", "small_runs")[3]
    assert [(n["need"], len(n["run"])) for n in small[::2]] == [(1, 5), (4, 5), (5, 5), (2, 3)]
    assert small[6]["run"][0] == 0 and small[6]["run"][-1] == 299
    equal = case("greedy", "all_equal")
    assert equal[3][0]["cut"] == 99 and len(equal[3][0]["run"]) == 1025 and equal[0][1] is None
    assert case("greedy", "all_equal_bias")[0][1] is not None
    assert case("greedy", "v_is_k_plus_1")[0][0].shape[1] == case("greedy", "v_is_k_plus_1")[1] + 1
    for name, pairs in (("top1_v1024", [(3, 40), (70, 700), (500, 1023)]), ("top1_v1025", [(0, 1024)]),
                        ("top1_v2049", [(7, 1031), (1000, 2048), (5, 2048)])):
        runs = [tuple(n["run"]) for n in case("greedy", name)[3] if n["family"] == "top-1"]
        assert all(p in runs for p in pairs)
    for name in ("v2500_k100_w8", "v2500_k8_w8"):                     # the beam: cut_w at column 1023, cut at column 1024
        notes = case("beam", name)[3]
        assert notes[0]["family"] == "w-run" and notes[0]["cut"] == BLOCK - 1 and notes[1]["probed"] == BLOCK
        assert sorted(set(c // BLOCK for c in notes[0]["run"])) == [0, 1, 2]
    assert case("beam", "v2500_k100_w8")[3][2]["cut"] == BLOCK
    assert set(case("beam", name)[2] for name in BEAM) == {2, 3, 8}
    for name in ("edges_v2500_k100_w8", "edges_v2500_k8_w8"):         # cut_w: a run longer than a block, the cut at 1024
        by_family = {n["family"]: n for n in case("beam", name)[3]}
        assert len(by_family["long-run"]["run"]) == 1500 and by_family["long-run"]["need"] == 5
        assert by_family["cut-at-block"]["cut"] == BLOCK and by_family["all-equal"]["cut"] == 7
    for name in (n for n in BEAM if n.startswith("edges")):           # all of the run fits; all but one of it
        notes = case("beam", name)[3]
        assert notes[0]["need"] == len(notes[0]["run"]) and notes[1]["need"] == len(notes[1]["run"]) - 1
    assert case("beam", "edges_v9_k8_w8")[0][0].shape[1] == case("beam", "edges_v9_k8_w8")[2] + 1


def test_the_shared_byte_rows_are_decided_by_their_low_key_bits():
    inputs, top_k, _, notes, _, _, _, _ = case("greedy", "shared_bytes")
    bits = sums_of(inputs).numpy().view(np.uint32)
    assert len(set((bits[0] >> 11).tolist())) == 1 and len(set((bits[2] >> 11).tolist())) == 1
    assert bool((sums_of(inputs)[0] > 0).all()) and bool((sums_of(inputs)[2] < 0).all())
    mixed = sums_of(inputs)[4]
    assert 0 < int((mixed > 0).sum()) < top_k and float(mixed[notes[4]["cut"]]) < 0


@pytest.mark.parametrize("kind,name,sample", [("greedy", "all_equal", 1), ("beam", "v37_k10_w3", 4)])
def test_the_input_condition_rejects_a_near_tie(kind, name, sample):
    inputs, top_k, W = case(kind, name)[:3]
    assert hold(inputs, top_k, W)[0]
    inputs = [t.clone() if t is not None else None for t in inputs]
    if kind == "greedy":
        inputs[0][sample, 100] += 1e-5                                # column 100 above the top-1, column 0, by 1e-5
    else:
        inputs[5][sample, 1] -= 1e-5                                  # parent 1 behind parent 0 by 1e-5, not level with it
    assert not hold(tuple(inputs), top_k, W)[0]


def test_every_case_is_run_on_the_gpu():
    import test_gpu_decode_ties as gpu
    assert sorted(gpu.GREEDY_NAMES) == sorted(GREEDY) and sorted(gpu.BEAM_NAMES) == sorted(BEAM)
    assert tie_cases.MARGIN == gpu.MARGIN
