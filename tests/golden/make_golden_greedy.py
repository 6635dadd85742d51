#!/usr/bin/env python
"""Generate tests/golden/greedy_*.npz from the REAL reference's GruCopyingDecoderModel.greedy_decode
(ptgnn/neuralmodels/sequence/grucopydecoder.py:375-457), imported unmodified and executed on CPU in fp32 around the
reference's own GruCopyingDecoder, with the shims of make_golden_decoder.py and two additions:
  * a stub vocabulary on the model (tests/greedy_cases.py StubVocabulary: `get_id_or_unk`, `get_name_for_id`; names
    t0 .. t{V-1}, except that the START and END ids carry the model's own "%START%" / "%END%");
  * `np.bool = bool` in this process (the reference predates numpy 1.24).

Runs only in the authoring container (the reference checkout does not travel to the GPU box).
    PYTHONHASHSEED=0 python tests/golden/make_golden_greedy.py

Cases and inputs: tests/greedy_cases.py.  A freshly initialised decoder scores all vocabulary entries within 1e-2 of each
other, so `tune_weights` spreads them first; the fixture holds the resulting state (`state.<reference key>`), the inputs,
the element ids, the reference's tokens as extended ids (`token_ids` [B, T] padded with -1, `lengths`) and its
log-probabilities (`logprobs`, float64); `spec` is the JSON of the case.  Every decision of every fixture must be at least
greedy_cases.MARGIN from flipping in the float64 restatement: a case that is not is refused here (pick another seed).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402  (installs the shims, puts the reference on sys.path)
import make_golden_decoder as D  # noqa: E402,F401  (the decoder's shims; imports the reference's module as D.ref)

from decoder_cases import build  # noqa: E402
from greedy_cases import (CASES, END_ID, MARGIN, START_ID, StubVocabulary, make_inputs, names_of, restated_decode,  # noqa: E402
                          tune_weights)

np.bool = bool


def main():
    for name, spec in CASES:
        gen = torch.Generator().manual_seed(9500 + spec["seed"])
        inputs = make_inputs(spec, gen)
        torch.manual_seed(spec["seed"])
        module = build(spec, D.ref).eval()
        tune_weights(module, gen)
        model = D.ref.GruCopyingDecoderModel(max_seq_len=spec["T"])
        model._GruCopyingDecoderModel__output_vocabulary = vocabulary = StubVocabulary(spec["V"])
        assert vocabulary.get_id_or_unk(model.START) == START_ID and vocabulary.get_name_for_id(END_ID) == model.END
        values = names_of(inputs["input_element_ids"], spec["V"])
        to_id = dict(zip(values, inputs["input_element_ids"].tolist()), **vocabulary.ids)
        with torch.no_grad():
            decoded = model.greedy_decode(
                input_concrete_values=values, input_memories=inputs["input_memories"],
                input_memories_origin_idx=inputs["input_memories_origin_idx"], initial_states=inputs["initial_states"],
                neural_model=module)
        tokens = np.full((spec["B"], spec["T"]), -1, dtype=np.int64)
        for b, (names, _) in enumerate(decoded):
            tokens[b, :len(names)] = [to_id[n] for n in names]
        lengths = np.asarray([len(names) for names, _ in decoded], dtype=np.int64)
        logprobs = np.asarray([float(p) for _, p in decoded], dtype=np.float64)
        w = {k.split("__", 1)[1]: v.double() for k, v in module.state_dict().items()}
        t64, l64, p64, gap, edge = restated_decode(w, inputs, spec)
        copies = int((tokens >= 0).sum() and sum(int(t in set(inputs["input_element_ids"].tolist())) for t in tokens[tokens >= 0]))
        print(f"{name}: gap {gap:.3e} edge {edge:.3e} lengths {np.bincount(lengths, minlength=spec['T'] + 1).tolist()} "
              f"tokens among the element ids {copies}/{int((tokens >= 0).sum())} outside the vocabulary "
              f"{int((tokens >= spec['V']).sum())} |logprob - f64| {np.abs(logprobs - p64).max():.2e}")
        assert gap >= MARGIN and edge >= MARGIN, (name, gap, edge)
        assert np.array_equal(tokens, t64) and np.array_equal(lengths, l64), name
        state = {"state." + k: v.detach().clone().numpy() for k, v in module.state_dict().items()}
        G.save(name, **{k: v.numpy() for k, v in inputs.items()}, spec=np.asarray(json.dumps(spec)), token_ids=tokens,
               lengths=lengths, logprobs=logprobs, **state)


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
