"""numpy restatement of tssa.label_histogram."""
import numpy as np


def label_histogram(target, num_classes, ignore_index=255):
    """int64 [num_classes]: the number of labels equal to c, labels equal to ignore_index or out of range left out."""
    t = np.asarray(target).reshape(-1)
    keep = (t >= 0) & (t < num_classes)
    if ignore_index is not None:
        keep &= t != ignore_index
    return np.bincount(t[keep], minlength=num_classes).astype(np.int64)
