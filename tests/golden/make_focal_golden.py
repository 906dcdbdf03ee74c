#!/usr/bin/env python
"""Generate tests/golden/focal.npz by running the REFERENCE's focal_loss itself (CPU, f32).

    python tests/golden/make_focal_golden.py <path to a checkout of the reference>

Only the arrays travel.  One 1x7x16x24 f32 input, about 10 % of the labels 255; the reference's loss and input gradient
for ignore_index=255, alpha=0.25 and gamma = 2.0 and 0.5.  tests/test_softloss_oracle.py pins tests/softloss_ref.py to
these numbers.  There is no Dice fixture: the reference's dice_loss raises on every call.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

B, C, H, W = 1, 7, 16, 24
GAMMAS = (2.0, 0.5)


def make_input():
    g = torch.Generator().manual_seed(4321)
    logits = 2.0 * torch.randn(B, C, H, W, generator=g)
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < 0.1] = 255
    return logits, target


def main(ref_root):
    sys.path.insert(0, ref_root)
    ref = importlib.import_module('torch_semantic_segmentation.losses.focal_loss')
    torch.set_num_threads(1)
    logits, target = make_input()
    assert 0.05 < (target == 255).float().mean() < 0.15
    out = {'logits': logits.numpy(), 'target': target.numpy().astype(np.int64)}
    for gamma in GAMMAS:
        x = logits.clone().requires_grad_(True)
        loss = ref.focal_loss(x, target, alpha=0.25, gamma=gamma, ignore_index=255)
        loss.backward()
        out['gamma%s/loss' % gamma] = loss.detach().numpy().astype(np.float32)
        out['gamma%s/grad' % gamma] = x.grad.numpy().astype(np.float32)
        print('gamma', gamma, 'loss', float(loss))
    np.savez_compressed(os.path.join(HERE, 'focal.npz'), **out)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
