"""ptgnn_amd -- MI355X-native message-passing core behind microsoft/ptgnn's layer API.

Only the hot path lives here: graph plan (CSR) construction, the fused
gather/segment-reduce kernel, fp32-MFMA dense blocks, and `nn.Module`s that mirror ptgnn's
`AbstractMessagePassingLayer` / `GraphNeuralNetwork` surface so `GnnOutput` consumers are drop-in.
"""
from ptgnn_amd._lib import PtgnnAmdError  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # `from ptgnn_amd import GruCopyingDecoder`: resolved on first use, so that importing the package stays as light as
    # it was (the layer modules are imported by their own names everywhere else)
    if name == "GruCopyingDecoder":
        from ptgnn_amd.sequence import GruCopyingDecoder
        return GruCopyingDecoder
    if name in ("Graph2ClassModule", "VarMisuseGraphModel", "PPIClassification", "Graph2SeqModule"):
        from ptgnn_amd import heads
        return getattr(heads, name)
    if name in ("TokenUnitEmbedder", "SubtokenUnitEmbedder", "CharUnitEmbedder", "CnnConfig", "LinearFeatureEmbedder"):
        from ptgnn_amd import embeddings
        return getattr(embeddings, name)
    if name in ("set_matrix_inputs", "get_matrix_inputs", "matrix_inputs", "edge_gemm_inputs", "training_inputs",
                "edge_training_inputs", "mlp_inputs", "attention_inputs"):
        from ptgnn_amd import precision
        return getattr(precision, name)
    raise AttributeError(f"module 'ptgnn_amd' has no attribute {name!r}")
