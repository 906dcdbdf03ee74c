"""tssa.label_histogram (csrc/labelhist.hip) against the restatement of tests/labelhist_ref.py: exact integer counts.  Label maps
are built on the CPU from fixed seeds: about 10 % labels 255 and a handful of out-of-range labels (-1, 300), which are not
counted."""
import functools

import numpy as np
import pytest
import torch

from tests import labelhist_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

#            B,  C,  H,  W, fraction of label 255, absent class
CASES = {
    'sub_wave':    (2, 19, 8, 24, 0.10, None),
    'two_blocks':  (1, 5, 48, 80, 0.10, 3),         # 480 groups of 8 labels: two blocks, the second ragged; class 3 absent
    'odd_batch':   (3, 21, 16, 40, 0.10, None),
    'two_classes': (2, 2, 8, 8, 0.10, None),
    'few_valid':   (2, 19, 32, 64, 0.995, None),
}


@functools.lru_cache(maxsize=None)
def case_target(name):
    B, C, H, W, frac, absent = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 500)
    target = torch.randint(0, C, (B, H, W), generator=g)
    if absent is not None:
        target[target == absent] = (absent + 1) % C
    target[torch.rand(B, H, W, generator=g) < frac] = 255
    flat = target.view(-1)
    flat[[3, 17, 40]] = -1
    flat[[5, 29]] = 300
    return target


@pytest.mark.parametrize('name', list(CASES))
def test_label_histogram_is_exact(name):
    import torch_semantic_segmentation_amd as tssa
    C = CASES[name][1]
    target = case_target(name)
    want = R.label_histogram(target, C, 255)
    t = target.to(DEV)
    got = tssa.label_histogram(t, C, ignore_index=255)
    assert got.dtype == torch.int64 and got.shape == (C,) and got.is_cuda
    assert got.cpu().numpy().tolist() == want.tolist() and want.sum() > 0
    again = tssa.label_histogram(t, C, ignore_index=255, out=got)        # accumulates into the caller's buffer
    assert again is got and got.cpu().numpy().tolist() == (2 * want).tolist()
    # another ignore index, none at all (255 is out of range either way), fewer classes than labels
    assert tssa.label_histogram(t, C, ignore_index=0).cpu().numpy().tolist() == R.label_histogram(target, C, 0).tolist()
    assert tssa.label_histogram(t, C, ignore_index=None).cpu().numpy().tolist() == R.label_histogram(target, C, None).tolist()
    assert tssa.label_histogram(t, 1, ignore_index=255).cpu().numpy().tolist() == R.label_histogram(target, 1, 255).tolist()


def test_label_histogram_over_several_blocks_and_odd_sizes():
    """1x1x64x2056: 16448 full pixel groups = 64 blocks and a quarter; 7x11x3 labels: a last group of 7; 300 classes."""
    import torch_semantic_segmentation_amd as tssa
    g = torch.Generator().manual_seed(21)
    target = torch.randint(0, 19, (1, 1, 64, 2056), generator=g)
    target[torch.rand(target.shape, generator=g) < 0.1] = 255
    target[0, 0, 10:30, 100:900] = 7                                     # a large uniform region: long runs of one label
    got = tssa.label_histogram(target.to(DEV), 19, ignore_index=255)
    assert got.cpu().numpy().tolist() == R.label_histogram(target, 19, 255).tolist()
    assert int(got.sum()) == int((target != 255).sum())
    odd = torch.randint(-2, 302, (7, 11, 3), generator=g)
    assert tssa.label_histogram(odd.to(DEV), 300, ignore_index=255).cpu().numpy().tolist() == R.label_histogram(odd, 300, 255).tolist()
    one = torch.randint(0, 2, (2, 8, 8), generator=g)
    assert tssa.label_histogram(one.to(DEV), 1).cpu().numpy().tolist() == [int((one == 0).sum())]
    assert tssa.label_histogram(torch.empty(0, dtype=torch.int64, device=DEV), 3).cpu().numpy().tolist() == [0, 0, 0]


def test_histogram_to_weights_recipe_and_errors():
    """label_histogram -> enet_class_weights on the device; argument errors."""
    import torch_semantic_segmentation_amd as tssa
    target = case_target('two_blocks')
    counts = tssa.label_histogram(target.to(DEV), 5, ignore_index=255)
    weight = tssa.enet_class_weights(counts)
    freq = R.label_histogram(target, 5, 255) / R.label_histogram(target, 5, 255).sum()
    want_w = 1.0 / np.log(1.02 + freq)
    assert weight.is_cuda and weight.dtype == torch.float32 and np.abs(weight.cpu().numpy() - want_w).max() <= 2.0 ** -23 * want_w.max()
    with pytest.raises(NotImplementedError):
        tssa.label_histogram(target.to(DEV), 5000)
    with pytest.raises(RuntimeError):
        tssa.label_histogram(target.to(DEV).int(), 5)
    with pytest.raises(RuntimeError):
        tssa.label_histogram(target.to(DEV), 5, out=torch.zeros(4, dtype=torch.int64, device=DEV))
