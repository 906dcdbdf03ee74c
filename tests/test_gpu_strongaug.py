"""tssa.strong_augment (csrc/strongaug.hip) against the float64 restatement tests/strongaug_ref.py, elementwise within its DERIVED
tolerance (that module's docstring; tests/test_strongaug_oracle.py shows, without a GPU, that the tolerance tells four wrong kernels
from the right one on these very cases).  B = 3, float32 and bfloat16, with and without mean / std, at 9x16 (every pixel reflects at
two borders at R = 8), 23x40 and (2 TH + 5) x (2 TW + 8) (ragged last tiles both ways); the row sets of strongaug_ref.row_sets rotate
over the samples with the size.  Every case also asserts: a second call gives the same bits, device rows and host rows give the same
bits, `out` given and out=None agree, identity samples (apply = 0, R = 0) come back on bits with a NaN planted in them.  Each case
prints a line `STRONGAUG_MARGIN case largest-bound median-bound largest-error/bound fallback-share` before it asserts
(profiles/strongaug_margins.txt)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import strongaug_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def tile():
    from torch_semantic_segmentation_amd import ops
    return ops.STRONGAUG_TILE


def _ids():
    from torch_semantic_segmentation_amd import ops
    return R.case_ids(ops.STRONGAUG_TILE)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def device_input(c, nan=()):
    x = torch.from_numpy(np.array(c['x']))
    for b in nan:                                  # samples that get a NaN planted: the identity ones
        x[b, 1, 2, 3] = float('nan')
    return x.to(DEV).to(torch.bfloat16 if c['bf16'] else torch.float32)       # the bf16 cases hold bf16 values already: exact


def test_tile_constant_matches_the_library():
    from torch_semantic_segmentation_amd import _native as N, ops
    th, tw = ctypes.c_int(), ctypes.c_int()
    assert N.lib().tss_strong_augment_tile(ctypes.byref(th), ctypes.byref(tw)) == 0
    assert (th.value, tw.value) == tuple(ops.STRONGAUG_TILE)


@pytest.mark.parametrize('case_id', _ids())
def test_against_the_restatement(case_id):
    import torch_semantic_segmentation_amd as tssa
    c = R.case(case_id, tile())
    want, tol, _ = R.reference(case_id, tile())
    identity = [w is None for w in want]
    x = device_input(c, nan=[b for b in range(3) if identity[b]])
    kw = dict(mean=c['mean'], std=c['std'])
    out = tssa.strong_augment(x, c['color'], c['radius'], c['taps'], **kw)
    assert out.dtype == x.dtype and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    again = tssa.strong_augment(x, c['color'], c['radius'], c['taps'], **kw)
    dev_rows = tssa.strong_augment(x, torch.from_numpy(c['color']).to(DEV), torch.from_numpy(c['radius']).to(DEV),
                                   torch.from_numpy(c['taps']).to(DEV), **kw)
    given = torch.full_like(x, 7.0)
    assert tssa.strong_augment(x, c['color'], c['radius'], c['taps'], out=given, **kw) is given
    got_bits = bits(out)
    for other in (again, dev_rows, given):
        assert np.array_equal(got_bits, bits(other))
    got = out.double().cpu().numpy()
    x_bits = bits(x)
    worst, bounds = 0.0, []
    for b in range(3):
        if identity[b]:
            assert np.array_equal(got_bits[b], x_bits[b]) and np.isnan(got[b, 1, 2, 3])
            continue
        assert np.isfinite(got[b]).all()
        worst = max(worst, float((np.abs(got[b] - want[b]) / tol[b]).max()))
        bounds.append(tol[b].ravel())
    if bounds:
        bounds = np.concatenate(bounds)
        print('STRONGAUG_MARGIN %s %.3e %.3e %.3f %.5f' % (case_id, bounds.max(), np.median(bounds), worst, R.fallback_share(case_id, tile())))
    assert worst <= 1.0, (case_id, worst)
    assert R.fallback_share(case_id, tile()) <= 0.01


def test_zero_contrast_gives_equal_channels():
    import torch_semantic_segmentation_amd as tssa
    for dt in ('f32', 'bf16'):
        case_id = 'degenerate-23x40-%s-raw' % dt
        c = R.case(case_id, tile())
        b = [i for i in range(3) if c['color'][i][2] == 0.0][0]
        out = tssa.strong_augment(device_input(c), c['color'], c['radius'], c['taps'])
        assert torch.equal(out[b, 0], out[b, 1]) and torch.equal(out[b, 1], out[b, 2]) and bool((out[b] == out[b, 0, 0, 0]).all())
        z = [i for i in range(3) if c['color'][i][1] == 0.0][0]             # fb = 0: black, m = 0
        assert bool((out[z] == 0).all())


def test_device_rows_are_clamped():
    """device rows are not validated: R = 11 runs as R = 8 and dh = 0.9 as 0.5 (taps w_0..w_8 are all there is)"""
    import torch_semantic_segmentation_amd as tssa
    c = R.case('mixed-23x40-f32-norm', tile())
    x = device_input(c)
    color = np.array(c['color'])
    color[:, 0], color[:, 4] = 1, 0.5
    radius = np.full(3, 8, np.int32)
    taps = np.stack([R.wide_taps(8)] * 3)
    want = tssa.strong_augment(x, color, radius, taps, mean=c['mean'], std=c['std'])
    color[:, 4] = 0.9
    got = tssa.strong_augment(x, torch.from_numpy(color).to(DEV), torch.full((3,), 11, dtype=torch.int32, device=DEV),
                              torch.from_numpy(taps).to(DEV), mean=c['mean'], std=c['std'])
    assert torch.equal(want, got)
    color[:, 4] = -0.9
    neg = tssa.strong_augment(x, torch.from_numpy(color).to(DEV), torch.full((3,), -3, dtype=torch.int32, device=DEV),
                              torch.from_numpy(taps).to(DEV), mean=c['mean'], std=c['std'])
    color[:, 4] = -0.5
    assert torch.equal(neg, tssa.strong_augment(x, color, np.zeros(3, np.int32), taps, mean=c['mean'], std=c['std']))


def test_contract_violations():
    import torch_semantic_segmentation_amd as tssa
    c = R.case('mixed-23x40-f32-raw', tile())
    x = device_input(c)
    rows = (c['color'], c['radius'], c['taps'])
    ok = tssa.strong_augment(x, *rows)

    def bad(*a, **k):
        with pytest.raises(ValueError):
            tssa.strong_augment(*a, **k)

    bad(torch.zeros((3, 1, 23, 40), device=DEV), *rows)                   # Ci != 3
    bad(torch.zeros((3, 3, 23, 36), device=DEV), *rows)                   # W % 8
    bad(torch.zeros((3, 3, 23, 8), device=DEV), *rows)                    # W < 16
    bad(torch.zeros((3, 3, 8, 40), device=DEV), *rows)                    # H < 9
    bad(x.double(), *rows)
    bad(x[:, :, :, ::2], *rows)                                           # not contiguous
    bad(x, *rows, out=x)                                                  # alias
    bad(x, *rows, out=torch.empty_like(x, dtype=torch.bfloat16))
    bad(x, *rows, out=torch.empty((3, 3, 23, 48), device=DEV))
    bad(x, c['color'][:2], c['radius'], c['taps'])
    bad(x, c['color'], c['radius'][:2], c['taps'])
    bad(x, c['color'], c['radius'], c['taps'][:, :9])
    bad(x, c['color'], np.array([0, 9, 1], np.int32), c['taps'])
    bad(x, c['color'], np.array([0, -1, 1], np.int32), c['taps'])
    bad(x, c['color'], c['radius'].astype(np.float32), c['taps'])
    for col, v in ((1, -0.1), (2, float('nan')), (3, float('inf')), (4, 0.6), (4, -0.6)):
        color = np.array(c['color'])
        color[1, col] = v
        bad(x, color, c['radius'], c['taps'])
    t = np.array(c['taps'])
    t[0, 0] = float('nan')
    bad(x, c['color'], c['radius'], t)
    bad(x, *rows, mean=(0.5, 0.5))
    bad(x, *rows, std=(1.0, 0.0, 1.0))
    bad(x, torch.from_numpy(c['color']).double().to(DEV), c['radius'], c['taps'])      # device rows: dtype is checked, values are not
    bad(x, *rows, workspace=torch.empty(4, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError):
        tssa.strong_augment(x.cpu(), *rows)
    assert torch.equal(ok, tssa.strong_augment(x, *rows))


def test_c_entry_refuses_a_short_image():
    from torch_semantic_segmentation_amd import _native as N
    lib = N.lib()
    x = torch.zeros((1, 3, 8, 16), device=DEV)
    out = torch.full_like(x, 3.0)
    color = torch.zeros((1, 8), device=DEV)
    radius = torch.zeros(1, dtype=torch.int32, device=DEV)
    taps = torch.zeros((1, 12), device=DEV)
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)
    args = lambda H, Ci=3, W=16: (x.data_ptr(), out.data_ptr(), color.data_ptr(), radius.data_ptr(), taps.data_ptr(), None, None,  # noqa: E731
                                  ws.data_ptr(), 1, Ci, H, W, N.TSS_F32, N.stream())
    assert lib.tss_strong_augment(*args(8)) == -2                          # TSS_ERR_SHAPE, nothing launched
    assert lib.tss_strong_augment(*args(9, Ci=1)) == -2 and lib.tss_strong_augment(*args(9, W=12)) == -2
    assert lib.tss_strong_augment_ws(1, 8, 16) == -1 and lib.tss_strong_augment_ws(2, 9, 16) == 2 * 64 * 8
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
