"""The matrix-core pool and copy scores past 8 heads (csrc/wide_heads.hip) without a GPU: the C ABI, the supported range,
the launch counters and the opt-in switch."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["wide_heads_pool", "wide_heads_pool_backward", "wide_heads_scores", "wide_heads_scores_backward"]


@pytest.fixture(scope="module")
def lib():
    from ptgnn_amd import _lib, build as B
    assert "wide_heads.hip" in B.SOURCES and os.path.exists(B.build())
    return _lib.load()


def test_header_signatures_and_library_agree(lib):
    from ptgnn_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptgnn_amd_wide_heads[a-z0-9_]*)\s*\(", text)))
    assert declared == sorted(["ptgnn_amd_wide_heads_supported", "ptgnn_amd_wide_heads_workspace_bytes"] +
                              [f"ptgnn_amd_{f}_f32" for f in FAMILIES])
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, s) for s in declared)
    assert sorted(s for s in _lib.SIGNATURES if "wide_heads" in s) == declared
    assert lib.ptgnn_amd_version() == 102


def test_supported_range_and_unsupported_calls(lib):
    from ptgnn_amd import _lib
    sup = lib.ptgnn_amd_wide_heads_supported
    assert [sup(256, h) for h in (0, 8, 9, 64, 65)] == [0, 0, 1, 1, 0]
    assert [sup(512, 32), sup(512, 33), sup(513, 9), sup(0, 16), sup(1, 9)] == [1, 0, 0, 0, 1]
    assert lib.ptgnn_amd_attention_pool_supported(256, 9) == 0 and lib.ptgnn_amd_segment_scores_supported(256, 9) == 0
    assert lib.ptgnn_amd_wide_heads_workspace_bytes(0, 1, 5, 1000, 256, 16) >= (1000 // 128 + 5) * 16 * 256 * 4
    for name in ("pool", "scores"):
        fwd, bwd = getattr(lib, f"ptgnn_amd_wide_heads_{name}_f32"), getattr(lib, f"ptgnn_amd_wide_heads_{name}_backward_f32")
        for dim, heads in ((256, 8), (256, 65), (512, 33)):
            rc = fwd(None, dim, None, None, None, 3, 10, dim, heads, None, None, None, 0, None)
            assert rc == _lib.EUNSUPPORTED and f"wide_heads_{name}:".encode() in lib.ptgnn_amd_last_error()
            tail = (None, None, None, None, dim, None, None, 0, None) if name == "pool" \
                else (None, None, None, None, None, dim, None, None, 0, None)
            rc = bwd(None, dim, None, None, None, 3, 10, dim, heads, *tail)
            assert rc == _lib.EUNSUPPORTED and f"wide_heads_{name}_backward:".encode() in lib.ptgnn_amd_last_error()


def test_counter_range_and_keyword(lib):
    from ptgnn_amd import ops
    names = [lib.ptgnn_amd_launch_name(1216 + i) for i in range(5)]
    assert names == [f.encode() for f in FAMILIES] + [None]
    assert lib.ptgnn_amd_launch_name(1152 + 3) is None                    # the range in front ends where it did
    plain, wide = ops.launch_counts(), ops.launch_counts(wide_heads=True)
    assert set(wide) == set(plain) | set(FAMILIES) and not set(plain) & set(FAMILIES)
    params = inspect.signature(ops.launch_counts).parameters
    assert params["wide_heads"].default is False and list(params)[-1] == "edge16_training"
    assert ops.launches_since(wide) == {}


def test_switch_is_off_by_default_and_the_context_manager_restores_it():
    import ptgnn_amd
    from ptgnn_amd import precision
    assert precision.get_wide_heads() is False
    with ptgnn_amd.wide_heads():
        assert ptgnn_amd.get_wide_heads() is True
        with ptgnn_amd.wide_heads(False):
            assert precision.get_wide_heads() is False
        assert precision.get_wide_heads() is True
    assert precision.get_wide_heads() is False
    assert ptgnn_amd.set_wide_heads(True) is False and ptgnn_amd.set_wide_heads(False) is True
    with ptgnn_amd.matrix_inputs("autocast"), ptgnn_amd.wide_heads():      # a setting of its own
        ptgnn_amd.set_matrix_inputs("autocast")
        assert precision.get_wide_heads() is True
