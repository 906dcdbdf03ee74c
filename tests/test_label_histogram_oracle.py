"""CPU checks of the label-histogram restatement and of tssa.enet_class_weights."""
import numpy as np
import torch

from tests import labelhist_ref as R

# class frequencies of the Cityscapes training set (19 classes), as data
CITYSCAPES_FREQ = (0.3687, 0.0608, 0.2282, 0.0066, 0.0088, 0.0123, 0.0021, 0.0055, 0.1593, 0.0116, 0.0402, 0.0122, 0.0014, 0.0699,
                   0.0027, 0.0024, 0.0023, 0.0010, 0.0041)


def test_histogram_restatement():
    t = torch.tensor([[0, 1, 1, 255, 3, -1, 300, 3, 3, 4]])
    assert R.label_histogram(t, 5, 255).tolist() == [1, 2, 0, 3, 1]
    assert R.label_histogram(t, 4, 255).tolist() == [1, 2, 0, 3]             # label 4 is out of range for 4 classes
    assert R.label_histogram(t, 5, 3).tolist() == [1, 2, 0, 0, 1]
    assert R.label_histogram(t, 5, None).tolist() == [1, 2, 0, 3, 1]
    assert R.label_histogram(t, 5, 255).dtype == np.int64


def test_enet_class_weights_recipe():
    """1 / log(1.02 + frequency) on the 19 Cityscapes frequencies; integer counts are normalized first."""
    import torch_semantic_segmentation_amd as tssa
    f = np.asarray(CITYSCAPES_FREQ, dtype=np.float64)
    assert f.shape == (19,) and abs(f.sum() - 1.0) < 1e-3
    want = 1.0 / np.log(1.02 + f)
    got = tssa.enet_class_weights(torch.from_numpy(f))
    assert got.dtype == torch.float32 and got.shape == (19,)
    assert np.abs(got.numpy() - want).max() <= 2.0 ** -23 * want.max()          # one rounding to f32
    # the reference's own line, in f32 throughout: rounding 1.02 + f (about 1.021 for the rarest class) to f32 moves the
    # logarithm 0.0208 by up to 2**-24 * 1.021 / 0.0208 = 2.9e-6 relative, and three more roundings follow
    got32 = tssa.enet_class_weights(torch.from_numpy(f.astype('f4')))
    assert np.abs(got32.numpy() - want).max() <= 1e-5 * want.max()
    counts = torch.tensor([600, 300, 100, 0])
    want = 1.0 / np.log(1.02 + np.array([0.6, 0.3, 0.1, 0.0]))
    got = tssa.enet_class_weights(counts)
    assert got.dtype == torch.float32 and np.abs(got.numpy() - want).max() <= 2.0 ** -23 * want.max()
    got = tssa.enet_class_weights(counts, c=1.1)
    want = 1.0 / np.log(1.1 + np.array([0.6, 0.3, 0.1, 0.0]))
    assert np.abs(got.numpy() - want).max() <= 2.0 ** -23 * want.max()
