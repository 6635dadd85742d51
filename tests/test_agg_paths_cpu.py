"""The degree-spectrum graph builder of tests/agg_paths.py (CPU only): it gives exactly the in-degrees it claims, and the
hub / chunk layout the GPU path tests (tests/test_gpu_aggregation_paths.py) rely on."""
import pytest
import torch

import agg_paths as AP


@pytest.mark.parametrize("num_types", [1, 3])
def test_spectrum_graph_has_the_requested_degrees_and_layout(num_types):
    sp = AP.spectrum_graph(num_types=num_types)
    N, E = sp.num_nodes, sp.num_edges
    src, dst, typ = sp.src_dst_type()
    assert len(sp.adj) == num_types and dst.shape[0] == E
    # exactly the requested in-degrees, every spectrum degree present
    assert torch.equal(torch.bincount(dst, minlength=N), sp.deg)
    present = set(sp.deg.tolist())
    assert all(d in present for d in AP.SPECTRUM_DEGREES), sorted(set(AP.SPECTRUM_DEGREES) - present)
    assert 6000 <= N <= 10000 and 30000 <= E <= 60000 and AP.HUB_THRESHOLD < E < (1 << 19)
    # hubs: row 0, row N-1 and an adjacent pair sharing a chunk
    hubs = sp.hub_rows
    r0, r1 = sp.shared_pair
    assert 0 in hubs and N - 1 in hubs and r0 in hubs and r1 == r0 + 1 and r1 in hubs
    assert set(sp.hub_chunks(r0)) & set(sp.hub_chunks(r1)), "the adjacent hubs do not share a chunk"
    assert int(sp.rowptr()[r1]) % AP.K_HUB_CHUNK != 0
    assert int(sp.deg[0]) == 3073 and int(sp.deg[N - 1]) == 2049
    # degrees exactly at and just past the thresholds, each with one row beyond a multiple of the unroll group
    for d in (AP.HUB_THRESHOLD, AP.HUB_THRESHOLD + 1, AP.K_LONG_ROW, AP.K_LONG_ROW + 1, AP.K_HUB_CHUNK + 1,
              AP.UNROLL + 1):
        assert d in present
    assert int((sp.deg > AP.HUB_THRESHOLD).sum()) == len(hubs) == 7   # 2049, 3073, 4097 + row 0, row N-1, the pair
    # messages are not in CSR order: the concatenated destinations are not sorted
    assert not bool((dst[1:] >= dst[:-1]).all())
    # a hub source: > HUB_THRESHOLD out-edges of type 0, so the backward plan (rows src * T + type) has a hub row
    out0 = int(((src == sp.hub_source) & (typ == 0)).sum())
    assert out0 > AP.HUB_THRESHOLD
    bdeg = torch.bincount(src * num_types + typ, minlength=N * num_types)
    assert int(bdeg.max()) == out0


def test_tie_values_hold_signed_zeros_in_every_column_class():
    v = AP.tie_values(4096, 7, seed=3)
    bits = v.view(torch.int32)
    neg0 = int(torch.tensor(-0.0).view(torch.int32))
    for c in range(7):
        col = v[:, c]
        assert bool((bits[:, c] == neg0).any()) and bool((bits[:, c] == 0).any())
        if c % 3 == 1:
            assert float(col.max()) == 0.0
        if c % 3 == 2:
            assert float(col.min()) == 0.0


def test_first_winner_returns_the_earliest_signed_zero():
    m = torch.tensor([[1.0], [-0.0], [0.0], [-1.0], [0.0], [-0.0]])
    t = torch.tensor([0, 0, 0, 1, 1, 1])
    val, arg = AP.first_winner(m, t, 3, "max")
    assert arg[:, 0].tolist() == [0, 4, 6]
    assert val[1, 0].view(torch.int32) == 0          # +0.0 at position 4 comes before -0.0 at 5
    val, arg = AP.first_winner(m, t, 3, "min")
    assert arg[:, 0].tolist() == [1, 3, 6]
    assert int(val[0, 0].view(torch.int32)) == int(torch.tensor(-0.0).view(torch.int32))
