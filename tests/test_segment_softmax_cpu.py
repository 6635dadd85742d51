"""The fused segment softmax without a GPU: it is built and declared, the ABI version stands, and the facade switch
changes nothing for CPU tensors."""
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_file_is_built_and_declared():
    from ptgnn_amd import _lib, build
    assert "segment_softmax.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "ptgnn_amd.h")).read()
    for name in ("ptgnn_amd_segment_softmax_supported", "ptgnn_amd_segment_softmax_workspace_bytes",
                 "ptgnn_amd_segment_softmax_state_f32", "ptgnn_amd_segment_softmax_write_f32"):
        assert name + "(" in header and name in _lib.SIGNATURES
    build.build()
    lib = _lib.load()
    assert lib.ptgnn_amd_version() == 102
    assert lib.ptgnn_amd_segment_softmax_supported(50, 100000, 8) == 1
    assert lib.ptgnn_amd_segment_softmax_supported(50, 1 << 31, 8) == 0
    assert lib.ptgnn_amd_segment_softmax_supported(1 << 20, 10, 1 << 11) == 0       # segments * dim = 2^31
    assert lib.ptgnn_amd_segment_softmax_workspace_bytes(50, 100000, 8, 0) > \
        lib.ptgnn_amd_segment_softmax_workspace_bytes(50, 100000, 8, 1) > 0


def test_switch_returns_the_previous_value_and_is_off_by_default():
    import ptgnn_amd
    from ptgnn_amd import scatter as S
    assert ptgnn_amd.set_fused_softmax is S.set_fused_softmax and ptgnn_amd.fused_softmax is S.fused_softmax
    assert S.set_fused_softmax(True) is False
    assert S.set_fused_softmax(False) is True
    with S.fused_softmax():
        with S.fused_softmax(False):
            assert S.set_fused_softmax(False) is False
        assert S.set_fused_softmax(True) is True
    assert S.set_fused_softmax(False) is False


def test_cpu_tensors_do_not_follow_the_switch():
    from ptgnn_amd import scatter as S
    g = torch.Generator().manual_seed(2)
    src = torch.randn(200, 5, generator=g)
    index = torch.randint(0, 30, (200,), generator=g)
    for name in ("scatter_softmax", "scatter_log_softmax", "scatter_logsumexp"):
        plain = getattr(S, name)(src, index, dim=0, dim_size=32)
        with S.fused_softmax():
            assert torch.equal(getattr(S, name)(src, index, dim=0, dim_size=32), plain)
