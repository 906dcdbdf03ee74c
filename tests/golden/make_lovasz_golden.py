#!/usr/bin/env python
"""Generate tests/golden/lovasz.npz by running the REFERENCE's lovasz_softmax_loss itself (CPU, f32).

    python tests/golden/make_lovasz_golden.py <path to a checkout of the reference>

Only the arrays travel.  One 1x7x16x24 f32 input, about 10 % of the labels 255, class 5 absent; the reference's
loss and input gradient for ignore_index=255 and for ignore_index=None (the 255 labels then stay in the pixel set as
background of every class).  tests/test_lovasz_oracle.py pins tests/lovasz_ref.py to these numbers.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

B, C, H, W = 1, 7, 16, 24
ABSENT = 5


def make_input():
    g = torch.Generator().manual_seed(1234)
    logits = 2.0 * torch.randn(B, C, H, W, generator=g)
    target = torch.randint(0, C - 1, (B, H, W), generator=g)
    target[target >= ABSENT] += 1                                   # classes 0..4 and 6: class 5 never occurs
    target[torch.rand(B, H, W, generator=g) < 0.1] = 255
    return logits, target


def main(ref_root):
    sys.path.insert(0, ref_root)
    ref = importlib.import_module('torch_semantic_segmentation.losses.lovasz_softmax_loss')
    torch.set_num_threads(1)
    logits, target = make_input()
    assert (target == ABSENT).sum() == 0 and 0.05 < (target == 255).float().mean() < 0.15
    out = {'logits': logits.numpy(), 'target': target.numpy().astype(np.int64)}
    for name, ignore in (('ignore255', 255), ('ignore_none', None)):
        x = logits.clone().requires_grad_(True)
        loss = ref.lovasz_softmax_loss(x, target, num_classes=C, ignore_index=ignore)
        loss.backward()
        out[name + '/loss'] = loss.detach().numpy().astype(np.float32)
        out[name + '/grad'] = x.grad.numpy().astype(np.float32)
        print(name, 'loss', float(loss))
    np.savez_compressed(os.path.join(HERE, 'lovasz.npz'), **out)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
