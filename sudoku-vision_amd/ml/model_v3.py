"""MI355X drop-in for the reference's ml/model_v3.py: `DigitCNNv3` keeps the state_dict keys, constructor and call protocol that
pipeline/run_v2.py:95-128 relies on; forward() runs the hand-written HIP kernels of csrc/k8_cnn_v3.hip (true f32 on the matrix pipe,
BatchNorm folded into the convolutions when the weights are packed).  Inference only, GPU only.

The submodules below exist to hold parameters and buffers under the reference's names, so that a reference checkpoint loads with
strict=True; none of them is ever called.  Not provided: DigitCNNv3Light, EmptyClassifier, calibrate_temperature (run_v2 uses none)."""
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _bootstrap import package  # noqa: E402
sys.path.pop(0)
_rt = package().runtime


def _conv_bn(cin, cout, k, stride):
    return [nn.Conv2d(cin, cout, kernel_size=k, stride=stride, padding=k // 2, bias=False), nn.BatchNorm2d(cout)]


class _Squeeze(nn.Module):
    """Holder of the two bias-free Linear layers of a squeeze-and-excitation gate, as `excite.0` and `excite.2`."""

    def __init__(self, channels):
        super().__init__()
        self.excite = nn.Sequential(nn.Linear(channels, channels // 4, bias=False), nn.ReLU(), nn.Linear(channels // 4, channels, bias=False), nn.Sigmoid())


class _Block(nn.Module):
    """Holder of one residual block's tensors: conv1/bn1, conv2/bn2, the optional gate `se`, and `shortcut` (1x1 conv + BN where the
    shape changes)."""

    def __init__(self, cin, cout, stride, use_se):
        super().__init__()
        self.conv1, self.bn1 = _conv_bn(cin, cout, 3, stride)
        self.conv2, self.bn2 = _conv_bn(cout, cout, 3, 1)
        self.se = _Squeeze(cout) if use_se else nn.Identity()
        self.shortcut = nn.Sequential(*_conv_bn(cin, cout, 1, stride)) if (stride != 1 or cin != cout) else nn.Identity()


class DigitCNNv3(nn.Module):
    """Residual digit classifier of the reference's ml/model_v3.py:95-149: stem, five residual blocks (32, 64/2, 64, 128/2, 128), global
    average pool, fc; `temperature` calibrates get_confidence."""

    def __init__(self, num_classes: int = 10, dropout: float = 0.5, use_se: bool = True):
        super().__init__()
        if num_classes != 10:
            raise NotImplementedError("the HIP forward is specialised for the reference's 10 classes")
        self.use_se = bool(use_se)
        self.stem = nn.Sequential(*_conv_bn(1, 32, 3, 1), nn.ReLU())
        for i, (cin, cout, stride) in enumerate(_rt._V3_BLOCKS, 1):
            setattr(self, f"layer{i}", _Block(cin, cout, stride, self.use_se))
        self.dropout = nn.Dropout(dropout)          # identity in eval mode, the only mode there is here
        self.fc = nn.Linear(128, num_classes)
        self.temperature = nn.Parameter(torch.ones(1), requires_grad=False)

    def _weights_key(self):
        # parameters AND BatchNorm buffers: running statistics are folded into the packed weights
        return tuple((v.data_ptr(), v._version) for v in self.state_dict(keep_vars=True).values())

    def _context(self, x):
        ctx = _rt._model_context(x, self.training, "DigitCNNv3", "dropout is identity and BatchNorm uses its running statistics")
        key = (id(self), self._weights_key())
        if ctx._weights_v3_key != key:
            ctx.load_state_dict_v3(self.state_dict(), use_se=self.use_se, key=key)
        return ctx

    def forward(self, x: torch.Tensor, return_features: bool = False) -> torch.Tensor:
        ctx = self._context(x)
        x = x.to(torch.float32).contiguous()
        if return_features:
            return ctx.cnn3_forward(x, want_features=True)[1]
        return ctx.cnn3_forward(x)

    def get_confidence(self, x: torch.Tensor):
        """(predicted class, softmax(logits / temperature) at it) -- reference ml/model_v3.py:216-225."""
        ctx = self._context(x)
        _, digits, conf = ctx.cnn3_forward(x.to(torch.float32).contiguous(), want_digits=True)
        return digits.to(torch.int64), conf

    def forward_with_uncertainty(self, x, n_samples: int = 10):
        raise NotImplementedError("DigitCNNv3 (MI355X): MC dropout needs train-mode dropout; this forward is inference only")

    def set_temperature(self, temperature: float):
        with torch.no_grad():
            self.temperature.fill_(temperature)         # in place on the parameter itself, so that its version (the re-pack key) moves


def count_parameters(model: nn.Module) -> int:
    """Count trainable parameters (reference ml/model_v3.py:323-325)."""
    return sum(p.numel() for p in model.parameters() if p.requires_grad)
