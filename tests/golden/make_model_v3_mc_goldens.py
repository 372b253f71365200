"""Writes tests/golden/model_v3_mc.npz: MC dropout of the REFERENCE's own ml/model_v3.py DigitCNNv3 (imported from the reference tree,
CPU f32) with BatchNorm on its running statistics -- the module is in eval mode, only `dropout` and `spatial_dropout` are in train mode,
and the self.train() of forward_with_uncertainty (:200) is made a no-op for the call, so that the reference's own sampling loop and
stacking code (:202-211) produce mean, std and predicted.  Forward hooks recover the keep masks the reference drew (a channel that is zero
before the dropout is recorded as kept: either bit gives the same output) and the per-sample logits (fc's output).
Seeds, the inputs' seed, masks and outputs only: the weights are regenerated from the seed.

Run where the reference tree is available:   python tests/golden/make_model_v3_mc_goldens.py <reference root>"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import model_v3_ref  # noqa: E402

W_SEED, X_SEED, B, S, TEMPERATURE, TORCH_SEED = 2024, 13, 3, 4, 1.7, 99


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "ml"))
    from model_v3 import DigitCNNv3
    torch.manual_seed(0)
    model = DigitCNNv3(use_se=True)
    sd = model_v3_ref.random_state_dict_v3(W_SEED, True)
    sd["temperature"] = torch.full((1,), TEMPERATURE)
    model.load_state_dict({**{k: v for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")}, **sd}, strict=True)
    model.eval()
    model.dropout.train()
    model.spatial_dropout.train()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    spatial, feature, logits = [], [], []

    def keep_of(inp, out, dims):
        return ((out != 0).flatten(dims).any(-1) | (inp == 0).flatten(dims).all(-1)).numpy().astype(np.uint8)

    model.spatial_dropout.register_forward_hook(lambda m, i, o: spatial.append(keep_of(i[0], o, 2)))
    model.dropout.register_forward_hook(lambda m, i, o: feature.append(keep_of(i[0][..., None], o[..., None], 2)))
    model.fc.register_forward_hook(lambda m, i, o: logits.append(o.detach().numpy().copy()))
    x = torch.from_numpy(model_v3_ref.inputs(X_SEED, B))
    model.train = lambda mode=True: model                  # :200 would put the BatchNorms on batch statistics
    torch.manual_seed(TORCH_SEED)
    with torch.no_grad():
        mean, std, predicted = model.forward_with_uncertainty(x, n_samples=S)
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items()), "the running statistics moved"
    keep1, keep3 = np.stack(spatial[0::2]), np.stack(spatial[1::2])
    keepf = np.stack(feature)
    assert keep1.shape == (S, B, 32) and keep3.shape == (S, B, 64) and keepf.shape == (S, B, 128)
    np.savez_compressed(os.path.join(HERE, "model_v3_mc.npz"), w_seed=W_SEED, x_seed=X_SEED, b=B, s=S, temperature=TEMPERATURE,
                        p_spatial=model.spatial_dropout.p, p_fc=model.dropout.p, keep1=keep1, keep3=keep3, keepf=keepf,
                        logits=np.stack(logits), mean=mean.numpy(), std=std.numpy(), predicted=predicted.numpy())
    print("kept", keep1.mean(), keep3.mean(), keepf.mean(), "predicted", predicted.numpy())


if __name__ == "__main__":
    main(sys.argv[1])
