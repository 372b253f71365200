"""Writes tests/golden/model_v3_light.npz and model_v3_empty.npz: outputs of the REFERENCE's own ml/model_v3.py DigitCNNv3Light and
EmptyClassifier (imported from the reference tree, eval mode, CPU f32) for the seeded weights and inputs of tests/model_v3_light_ref.py,
plus the key names, shapes and dtypes of their state_dicts and their trainable-parameter counts.  Seeds and outputs only: the weights are
regenerated from the seed.

Run where the reference tree is available:   python tests/golden/make_model_v3_light_goldens.py [reference root, default /root/reference]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import model_v3_light_ref as ref  # noqa: E402

W_SEED, X_SEED, N = 2024, 7, 48


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "ml"))
    from model_v3 import DigitCNNv3Light, EmptyClassifier
    for cls, make, name in ((DigitCNNv3Light, ref.random_state_dict_light, "light"), (EmptyClassifier, ref.random_state_dict_empty, "empty")):
        torch.manual_seed(0)
        model = cls()
        full = model.state_dict()
        sd = make(W_SEED)
        model.load_state_dict({**{k: v for k, v in full.items() if k.endswith("num_batches_tracked")}, **sd}, strict=True)
        model.eval()
        x = torch.from_numpy(ref.inputs(X_SEED, N))
        with torch.no_grad():
            out = model(x).numpy()
        np.savez_compressed(os.path.join(HERE, f"model_v3_{name}.npz"), w_seed=W_SEED, x_seed=X_SEED, n=N, logits=out,
                            keys=np.array(list(full.keys())), shapes=np.array([",".join(map(str, v.shape)) for v in full.values()]),
                            dtypes=np.array([str(v.dtype) for v in full.values()]),
                            n_parameters=sum(p.numel() for p in model.parameters() if p.requires_grad))
        print(name, out.shape, len(full), "keys")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
