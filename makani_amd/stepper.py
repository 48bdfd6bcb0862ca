"""The model wrappers the trainer and the inferencer call instead of the network: ``SingleStepWrapper`` and
``MultiStepWrapper`` of ``makani/models/stepper.py`` -- same constructors ``(params, model_handle)``, same attributes
``.preprocessor`` and ``.model`` (so the ``state_dict`` keys are the reference's ``model.*``; the preprocessor's buffers
are non-persistent), same ``forward``.

The reference's four preprocessing calls before every model call (``append_unpredicted_features``,
``history_compute_stats``, ``history_normalize``, ``add_static_features``) are one ``Preprocessor2D.assemble`` here: one
HIP pass on CUDA tensors, the same torch ops otherwise (see ``preprocessor.py``).  When bf16 autocast is on and the model
is this package's SFNO under the conditions where its ``_forward`` would cast the fp32 input for the pixel-column engine
anyway, the pass writes that bf16 field directly; the model output is then bit-identical to feeding it the fp32
assembly.  In every other case the assembled input is fp32.

Deviations from the reference (a fork with local edits), keeping the evident intent:

* ``stepper.py:45,60`` hard-code a land-sea mask on channel 20 of sample 0 of the input and of the denormalised output.
  Here ``params.masked_channels`` names the channels (default none, which is upstream behaviour) and the mask applies to
  all samples: the input side inside the assemble pass, the output side as a torch op on those channels
  (``Preprocessor2D.mask_output``), in both wrappers.
* ``MultiStepWrapper.forward`` raises in the fork (line 149); here it runs ``_forward_train`` in training mode, whose
  ``n_future + 1`` predictions are concatenated along the channels as ``LossHandler``'s multistep weights expect, and
  ``_forward_eval`` otherwise.
* ``SingleStepWrapper`` calls ``add_residual`` as upstream does (the fork commented it out; it is a no-op for
  ``target: "default"``).
* ``history_denormalize`` works in the statistics modes and ``add_residual`` is out of place (``preprocessor.py``).
"""
import torch
from torch import nn

from . import ops
from .preprocessor import Preprocessor2D


def _engine_input_dtype(model, inp):
    """bf16 when ``model`` would cast its fp32 input to the bf16 engine field first thing (the conditions of
    ``SphericalFourierNeuralOperatorNet._forward`` and ``layers._engine_field``), else None (fp32)."""
    from .sfnonet import SphericalFourierNeuralOperatorNet
    if not isinstance(model, SphericalFourierNeuralOperatorNet):
        return None
    if not (inp.is_cuda and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16):
        return None
    if not (model.big_skip and model.out_shape == model.inp_shape and (inp.shape[-2] * inp.shape[-1]) % 8 == 0):
        return None
    if ops._knob("MK_CONV_ENGINE", "pce") != "pce":
        return None
    return torch.bfloat16


class SingleStepWrapper(nn.Module):
    def __init__(self, params, model_handle):
        super().__init__()
        self.preprocessor = Preprocessor2D(params)
        self.model = model_handle()

    def forward(self, inp):
        # unpredicted features, history normalisation, static features and mask in one pass
        inpans = self.preprocessor.assemble(inp, out_dtype=_engine_input_dtype(self.model, inp))
        yn = self.model(inpans)
        # undo the normalisation, mask the denormalised output
        y = self.preprocessor.history_denormalize(yn, target=True)
        y = self.preprocessor.mask_output(y)
        # add residual (for residual learning, no-op for direct learning)
        return self.preprocessor.add_residual(inp, y)


class MultiStepWrapper(nn.Module):
    def __init__(self, params, model_handle):
        super().__init__()
        self.preprocessor = Preprocessor2D(params)
        self.model = model_handle()
        self.residual_mode = True if (params.target == "target") else False
        self.n_future = params.n_future

    def _step(self, inp):
        inpans = self.preprocessor.assemble(inp, out_dtype=_engine_input_dtype(self.model, inp))
        predn = self.model(inpans)
        # denormalise here: the statistics are updated by the next step's assembly
        pred = self.preprocessor.history_denormalize(predn, target=True)
        pred = self.preprocessor.mask_output(pred)
        return self.preprocessor.add_residual(inp, pred)

    def _forward_train(self, inp):
        result = []
        inpt = inp
        for step in range(self.n_future + 1):
            pred = self._step(inpt)
            result.append(pred)
            if step == self.n_future:
                break
            inpt = self.preprocessor.append_history(inpt, pred, step)
        # concatenated along the channels to be compatible with the flattened target
        return torch.cat(result, dim=1)

    def _forward_eval(self, inp):
        return self._step(inp)

    def forward(self, inp):
        return self._forward_train(inp) if self.training else self._forward_eval(inp)
