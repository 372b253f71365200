"""MI355X drop-in for the reference's ml/model_v3.py: `DigitCNNv3` keeps the state_dict keys, constructor and call protocol that
pipeline/run_v2.py:95-128 relies on; forward() runs the hand-written HIP kernels of csrc/k8_cnn_v3.hip (true f32 on the matrix pipe,
BatchNorm folded into the convolutions when the weights are packed).  `DigitCNNv3Light` and `EmptyClassifier` do the same through
csrc/k12_cnn_v3_light.hip, one launch per forward.  Forward only, GPU only.  `calibrate_temperature` is plain torch on the logits; the ECE it is meant
to lower, and every other evaluation metric, is ml/evaluate_v2.py's (csrc/k21_eval.hip).

The submodules below exist to hold parameters and buffers under the reference's names, so that a reference checkpoint loads with
strict=True; none of them is ever called.

`DigitCNNv3.forward_with_uncertainty` is MC dropout on the GPU (csrc/k8_cnn_v3.hip, sv_cnn3_forward_mc_f32): the three dropouts of the
reference's forward (ml/model_v3.py:167, :170, :181) are active, BatchNorm is not -- where the reference's self.train() (:200) also puts
its BatchNorms on batch statistics and overwrites their running buffers, this one leaves the model as it was.  Its masks come from a
counter-based generator seeded by torch's CUDA generator, not from PyTorch's own draw order."""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

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


class SpatialDropout2d(nn.Module):
    """Holder of the rate of the reference's spatial dropout (ml/model_v3.py:80-92): whole feature maps are dropped at rate `p`, the kept
    ones scaled by 1 / (1 - p).  No parameters; forward_with_uncertainty reads `p`."""

    def __init__(self, p: float = 0.5):
        super().__init__()
        self.p = p


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
        self.spatial_dropout = SpatialDropout2d(p=0.1)   # after layer1 and layer3; active in forward_with_uncertainty alone
        self.dropout = nn.Dropout(dropout)          # identity in forward(); forward_with_uncertainty reads its p
        self.fc = nn.Linear(128, num_classes)
        self.temperature = nn.Parameter(torch.ones(1), requires_grad=False)

    def _weights_key(self):
        # parameters AND BatchNorm buffers: running statistics are folded into the packed weights
        return tuple((v.data_ptr(), v._version) for v in self.state_dict(keep_vars=True).values())

    def _context(self, x, mc_dropout=False):
        # mc_dropout: forward_with_uncertainty, the one caller that a module in training mode may reach the kernels through
        ctx = _rt._model_context(x, self.training and not mc_dropout, "DigitCNNv3", "dropout is identity and BatchNorm uses its running statistics")
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

    def forward_with_uncertainty(self, x: torch.Tensor, n_samples: int = 10, *, generator=None):
        """MC dropout (reference ml/model_v3.py:186-214): (mean, unbiased std, argmax of the mean) of softmax(logits / temperature) over
        n_samples forwards with `spatial_dropout` (after layer1 and layer3) and `dropout` (on the pooled features) drawing fresh masks,
        BatchNorm on its running statistics.  The masks are a function of the seed and offset of `generator` (default: the device's
        CUDA generator, so torch.manual_seed makes a call repeatable), which the call advances; a cell's masks do not depend on the rest
        of the batch.  Leaves the module in eval mode, as the reference does."""
        if int(n_samples) < 1:
            raise ValueError(f"n_samples must be at least 1, got {n_samples}")
        p_spatial, p_fc = float(self.spatial_dropout.p), float(self.dropout.p)
        if not 0.0 <= p_spatial < 1.0:
            raise ValueError(f"spatial_dropout.p must be in [0, 1), got {p_spatial}")
        if not 0.0 <= p_fc <= 1.0:
            raise ValueError(f"dropout.p must be in [0, 1], got {p_fc}")
        if not x.is_cuda:
            raise NotImplementedError("DigitCNNv3 (MI355X): forward_with_uncertainty runs on the GPU only; there is no CPU fallback")
        ctx = self._context(x, mc_dropout=True)
        gen = generator if generator is not None else torch.cuda.default_generators[x.device.index]
        seed, offset = gen.initial_seed(), gen.get_offset()
        gen.set_offset(offset + 4)
        out = ctx.cnn3_forward_mc(x.to(torch.float32).contiguous(), n_samples, p_spatial, p_fc, seed, offset)
        self.eval()
        return out

    def set_temperature(self, temperature: float):
        with torch.no_grad():
            self.temperature.fill_(temperature)         # in place on the parameter itself, so that its version (the re-pack key) moves


def _state_key(module):
    # parameters AND BatchNorm buffers: running statistics are folded into the packed weights
    return (id(module), tuple((v.data_ptr(), v._version) for v in module.state_dict(keep_vars=True).values()))


class DigitCNNv3Light(nn.Module):
    """The lighter digit classifier of the reference's ml/model_v3.py:232-282: three conv + BatchNorm + ReLU stages (24, 48, 96 channels,
    the first two max-pooled), global average pool, fc; `temperature` calibrates get_confidence."""

    def __init__(self, num_classes: int = 10, dropout: float = 0.5):
        super().__init__()
        if num_classes != 10:
            raise NotImplementedError("the HIP forward is specialised for the reference's 10 classes")
        self.features = nn.Sequential(*_conv_bn(1, 24, 3, 1), nn.ReLU(inplace=True), nn.MaxPool2d(2, 2),
                                      *_conv_bn(24, 48, 3, 1), nn.ReLU(inplace=True), nn.MaxPool2d(2, 2),
                                      *_conv_bn(48, 96, 3, 1), nn.ReLU(inplace=True))
        self.gap = nn.AdaptiveAvgPool2d(1)
        self.dropout = nn.Dropout(dropout)          # identity in eval mode, the only mode there is here
        self.fc = nn.Linear(96, num_classes)
        self.temperature = nn.Parameter(torch.ones(1), requires_grad=False)

    def _context(self, x):
        ctx = _rt._model_context(x, self.training, "DigitCNNv3Light", "dropout is identity and BatchNorm uses its running statistics")
        key = _state_key(self)
        if ctx._weights_light_key != key:
            ctx.load_state_dict_v3_light(self.state_dict(), key=key)
        return ctx

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._context(x).cnn3_light_forward(x.to(torch.float32).contiguous())

    def get_confidence(self, x: torch.Tensor):
        """(predicted class, softmax(logits / temperature) at it) -- reference ml/model_v3.py:278-282."""
        _, digits, conf = self._context(x).cnn3_light_forward(x.to(torch.float32).contiguous(), want_digits=True)
        return digits.to(torch.int64), conf

    def set_temperature(self, temperature: float):
        with torch.no_grad():
            self.temperature.fill_(temperature)         # in place on the parameter itself, so that its version (the re-pack key) moves


class EmptyClassifier(nn.Module):
    """The empty-cell classifier of the reference's ml/model_v3.py:285-320: two conv + ReLU + maxpool stages (16, 32 channels, with bias),
    Linear(1568, 32) + ReLU, Linear(32, 1); forward returns the logit, is_empty thresholds its sigmoid."""

    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(nn.Conv2d(1, 16, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(2, 2),
                                      nn.Conv2d(16, 32, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(2, 2))
        self.classifier = nn.Sequential(nn.Flatten(), nn.Linear(32 * 7 * 7, 32), nn.ReLU(inplace=True), nn.Dropout(0.3), nn.Linear(32, 1))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        ctx = _rt._model_context(x, self.training, "EmptyClassifier", "dropout is identity")
        key = _state_key(self)
        if ctx._weights_empty_key != key:
            ctx.load_state_dict_empty(self.state_dict(), key=key)
        return ctx.empty_forward(x.to(torch.float32).contiguous())

    def is_empty(self, x: torch.Tensor, threshold: float = 0.5) -> torch.Tensor:
        """Boolean [batch, 1]: the cells judged empty (reference ml/model_v3.py:317-320)."""
        return torch.sigmoid(self.forward(x)) < threshold


def calibrate_temperature(model: nn.Module, val_loader, device, lr: float = 0.01, max_iter: int = 50) -> float:
    """The temperature that minimises the negative log-likelihood of softmax(logits / T) on a validation set (reference
    ml/model_v3.py:328-371): the model's logits over val_loader's (data, target) batches are gathered once, then one LBFGS step of up to
    max_iter iterations runs on cross_entropy(logits / T, labels) from T = 1.5.  Calls nothing of the model but eval() and forward."""
    model.eval()
    gathered, targets = [], []
    with torch.no_grad():
        for data, target in val_loader:
            gathered.append(model(data.to(device)))
            targets.append(target.to(device))
    logits, labels = torch.cat(gathered), torch.cat(targets)
    t = nn.Parameter(torch.full((1,), 1.5, device=device))
    opt = torch.optim.LBFGS([t], lr=lr, max_iter=max_iter)

    def closure():
        opt.zero_grad()
        loss = F.cross_entropy(logits / t, labels)
        loss.backward()
        return loss

    opt.step(closure)
    value = t.item()
    print(f"Calibrated temperature: {value:.4f}")
    return value


def count_parameters(model: nn.Module) -> int:
    """Count trainable parameters (reference ml/model_v3.py:323-325)."""
    return sum(p.numel() for p in model.parameters() if p.requires_grad)
