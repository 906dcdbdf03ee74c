"""GPU: multi-scale + flip evaluation (csrc/msflip.hip) -- tss_multiscale_argmax_confusion against the float64 restatement
tests/msflip_ref.py (pinned by tests/test_msflip_oracle.py) wherever the restatement's top-2 gap exceeds the DERIVED score
margin (both scores may move by it, so exact arithmetic promises agreement only past twice it; the stricter single margin is what is
asserted, and the margin is some forty times what float32 arithmetic on these inputs is off by), the confusion counts exactly, tss_resize_flip_planar bit for bit against resize_image, the contract, and
engine.MultiScaleEvaluator end to end on FastSCNN."""
import ctypes
import functools

import pytest
import torch

from tests import cases
from tests import msflip_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# name -> (map sizes, output size); every size appears plain and flipped
GEOMETRY = {
    'twelve': (R.SIZES, R.OUT),                                                  # a map with h = H, w = W and a 1 x 1 map included
    'odd': (((5, 9), (3, 4), (8, 16), (10, 18), (33, 70), (1, 1)), (33, 70)),    # W % 8 != 0, odd H, a band with one row
    'single': (((5, 9),), (40, 72)),                                             # plain + flipped of one map
}
DTYPES = {'bf16': torch.bfloat16, 'f32': torch.float32}


@functools.lru_cache(maxsize=None)
def inputs(geometry, C):
    sizes, out = GEOMETRY[geometry]
    return R.make_maps(sizes, B=2, C=C, seed=0), out


@functools.lru_cache(maxsize=None)
def reference(geometry, C, average, pick=None):
    """(f64 arg-max, decided mask, margin); `pick` selects a subset of the maps (indices)."""
    (lows, flips), out = inputs(geometry, C)
    if pick is not None:
        lows, flips = [lows[i] for i in pick], [flips[i] for i in pick]
    score, pred = R.scores(lows, flips, out, average)
    zmax = max(float(low.abs().max()) for low in lows)
    m = R.margin(len(lows), C, zmax, [tuple(low.shape[-2:]) for low in lows], out, average)
    return pred, R.top2_gap(score) > m, m


def check(pred, geometry, C, average, pick, what):
    want, decided, m = reference(geometry, C, average, pick)
    pred = pred.cpu().long()
    excluded = 1.0 - float(decided.double().mean())
    wrong = int(((pred != want) & decided).sum())
    print('%s: margin %.3e, undecided share %.4f, wrong among decided %d, differing anywhere %d'
          % (what, m, excluded, wrong, int((pred != want).sum())))
    assert 2 * m <= 1e-3                                   # the range in which the gap statistics of these inputs were taken
    assert excluded <= 0.01
    assert wrong == 0


def fused(lows, flips, out, dtype, average, **kw):
    import torch_semantic_segmentation_amd as tssa
    return tssa.multiscale_argmax_confusion([low.to(DEV, dtype) for low in lows], flips, size=out, average=average, **kw)


@pytest.mark.parametrize('average', ['softmax', 'logits'])
@pytest.mark.parametrize('dtype', ['bf16', 'f32'])
@pytest.mark.parametrize('C', [19, 21, 3])
@pytest.mark.parametrize('geometry', ['twelve', 'odd'])
def test_fused_prediction_matches_the_restatement(geometry, C, dtype, average):
    (lows, flips), out = inputs(geometry, C)
    pred, cm = fused(lows, flips, out, DTYPES[dtype], average)
    assert cm is None and pred.dtype == torch.uint8 and tuple(pred.shape) == (2,) + tuple(out)
    check(pred, geometry, C, average, None, '%s C=%d %s %s' % (geometry, C, dtype, average))
    if geometry == 'twelve':
        # the same twelve descriptors as six 2B tensors (plain half, mirrored half) with flips (False, True): identical
        packed = [torch.cat([lows[i], lows[i + 1]]) for i in range(0, len(lows), 2)]
        pred2, _ = fused(packed, [(False, True)] * len(packed), out, DTYPES[dtype], average)
        assert torch.equal(pred2, pred)


@pytest.mark.parametrize('average', ['softmax', 'logits'])
@pytest.mark.parametrize('case,geometry,pick', [('K=1', 'single', (0,)), ('flip only', 'single', (1,)),
                                                ('h=H w=W', 'twelve', (8,)), ('h=H w=W flipped', 'twelve', (9,))])
def test_single_map_cases(case, geometry, pick, average):
    (lows, flips), out = inputs(geometry, 19)
    pred, _ = fused([lows[i] for i in pick], [flips[i] for i in pick], out, torch.bfloat16, average)
    check(pred, geometry, 19, average, pick, '%s %s' % (case, average))


@pytest.mark.parametrize('average', ['softmax', 'logits'])
def test_ties_go_to_the_lowest_index(average):
    lows = [torch.zeros(2, 19, 5, 9), torch.zeros(2, 19, 3, 4)]
    pred, _ = fused(lows, [False, True], (33, 70), torch.float32, average)
    assert int(pred.max()) == 0


@pytest.mark.parametrize('C', [19, 21])
def test_confusion_matrix_is_exact(C):
    (lows, flips), out = inputs('odd', C)
    g = torch.Generator().manual_seed(3)
    target = torch.randint(0, C, (2,) + tuple(out), generator=g)
    target[torch.rand(target.shape, generator=g) < 0.1] = 255
    target[0, 0, :5] = C                                   # out of range: skipped like ignore_index
    target[1, -1, -3:] = -2
    td = target.to(DEV)
    pred, cm = fused(lows, flips, out, torch.bfloat16, 'softmax', target=td)
    assert cm.dtype == torch.int64 and tuple(cm.shape) == (C, C)
    want = R.confusion(pred.cpu(), target, C)
    assert torch.equal(cm.cpu(), want)
    assert int(cm.sum()) == int(((target >= 0) & (target < C)).sum())
    pred2, cm2 = fused(lows, flips, out, torch.bfloat16, 'softmax', target=td, confusion=cm.clone(), want_pred=False)
    assert pred2 is None and torch.equal(cm2.cpu(), 2 * want)
    pred3, cm3 = fused(lows, flips, out, torch.bfloat16, 'softmax')
    assert cm3 is None and torch.equal(pred3, pred)


@pytest.mark.parametrize('size', [(48, 96), (16, 32), (32, 64), (21, 50)])
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_resize_flip_image_is_resize_image_and_its_mirror(size, dtype):
    from torch_semantic_segmentation_amd import ops
    from oracle.recipe import lattice_input
    x = lattice_input(2, 3, 32, 64).to(DEV)
    y = ops.resize_flip_image(x, size, out_dtype=DTYPES[dtype])
    ref = ops.resize_image(x, size=size, out_dtype=DTYPES[dtype])
    assert y.dtype == DTYPES[dtype] and tuple(y.shape) == (4, 3) + tuple(size)
    assert torch.equal(y[:2].cpu(), ref.cpu())
    assert torch.equal(y[2:].cpu(), ref.cpu().flip(-1))
    if tuple(size) == (32, 64) and dtype == 'f32':
        assert torch.equal(y[:2], x)                       # identity: the taps are exact
    plain = ops.resize_flip_image(x, size, flip=False, out_dtype=DTYPES[dtype])
    assert tuple(plain.shape) == (2, 3) + tuple(size) and torch.equal(plain.cpu(), ref.cpu())


def test_contract_errors():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import _native as N, ops
    low = torch.zeros(2, 19, 5, 9, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match='at least one map'):
        tssa.multiscale_argmax_confusion([], [], size=(40, 72))
    with pytest.raises(ValueError, match='at most 16 maps'):
        tssa.multiscale_argmax_confusion([low] * 17, [False] * 17, size=(40, 72))
    with pytest.raises(ValueError, match='at most 16 maps'):
        tssa.multiscale_argmax_confusion([torch.cat([low, low])] * 9, [(False, True)] * 9, size=(40, 72))
    with pytest.raises(ValueError, match='larger than the output'):
        tssa.multiscale_argmax_confusion([low], [False], size=(40, 8))
    with pytest.raises(ValueError, match='share dtype, device and class count'):
        tssa.multiscale_argmax_confusion([low, low.float()], [False, False], size=(40, 72))
    with pytest.raises(ValueError, match='share dtype, device and class count'):
        tssa.multiscale_argmax_confusion([low, low.cpu()], [False, False], size=(40, 72))
    with pytest.raises(ValueError, match='share dtype, device and class count'):
        tssa.multiscale_argmax_confusion([low, low[:, :3]], [False, False], size=(40, 72))
    with pytest.raises(ValueError, match="average must be"):
        tssa.multiscale_argmax_confusion([low], [False], size=(40, 72), average='mean')
    # a host map that is already channels-last (C % 8 == 0: to_nhwc hands it on as it is) must never reach the kernel
    host = torch.zeros(2, 8, 5, 9, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match='HIP path only'):
        tssa.multiscale_argmax_confusion([host], [False], size=(40, 72))

    # the C entry itself: TSS_ERR_SHAPE for K = 17 and for a map wider than the output, and nothing is launched
    nhwc = ops.to_nhwc(low)
    pred = torch.full((2, 40, 72), 7, dtype=torch.uint8, device=DEV)
    entry = N.lib().tss_multiscale_argmax_confusion
    N.prof_enable(True)
    try:
        N.prof_reset()
        maps = (ops._MsMap * 17)(*[ops._MsMap(nhwc.data_ptr(), ops.ld(nhwc), 5, 9, 0, 0) for _ in range(17)])
        assert entry(maps, 17, None, pred.data_ptr(), None, 2, 19, 40, 72, 255, 0, N.TSS_BF16, N.stream()) == -2
        assert entry(maps, 0, None, pred.data_ptr(), None, 2, 19, 40, 72, 255, 0, N.TSS_BF16, N.stream()) == -2
        assert entry(maps, 1, None, pred.data_ptr(), None, 2, 19, 40, 8, 255, 0, N.TSS_BF16, N.stream()) == -2     # w = 9 > W = 8
        assert entry(maps, 1, None, pred.data_ptr(), None, 2, 25, 40, 72, 255, 0, N.TSS_BF16, N.stream()) == -2    # C > 24
        assert entry(maps, 1, None, pred.data_ptr(), None, 2, 19, 40, 72, 255, 2, N.TSS_BF16, N.stream()) == -2    # unknown mode
        odd = (ops._MsMap * 1)(ops._MsMap(nhwc.data_ptr() + 2, ops.ld(nhwc), 5, 9, 0, 0))
        assert entry(odd, 1, None, pred.data_ptr(), None, 2, 19, 40, 72, 255, 0, N.TSS_BF16, N.stream()) == -3
        assert entry(maps, 1, None, pred.data_ptr(), None, 0, 19, 40, 72, 255, 0, N.TSS_BF16, N.stream()) == 0     # empty work
        assert N.prof_table() == {}
    finally:
        N.prof_enable(False)
        N.prof_reset()
    assert int(pred.min()) == 7 and int(pred.max()) == 7


@functools.lru_cache(maxsize=None)
def _model():
    from oracle.recipe import formula_state
    m = cases.product_model('fastscnn')
    m.load_state_dict(formula_state(m))
    return m.to(DEV).eval()


def test_multiscale_evaluator_end_to_end():
    import torch_semantic_segmentation_amd as tssa
    from torch_semantic_segmentation_amd import engine as E, ops
    from oracle.recipe import lattice_input, lattice_target
    model = _model()
    batches = [(lattice_input(2, 3, 64, 128).mul(1.0 + 0.25 * i), lattice_target(2, 64, 128).roll(i, -1)) for i in range(2)]
    ev = E.create_segmentation_evaluator(model, DEV, scales=(0.5, 1.0, 1.5), flip=True)
    assert isinstance(ev, tssa.MultiScaleEvaluator) and ev.average == 'softmax'
    assert [ev.scaled_size(64, 128, s) for s in ev.scales] == [(32, 64), (64, 128), (96, 192)]
    assert ev.scaled_size(64, 128, 0.1) == (32, 32)
    met = ev.run(batches)

    cm, preds = None, []
    with torch.no_grad(), E.EvalPrep(model):
        for x, y in batches:
            x, y = x.to(DEV), y.to(DEV)
            lows = [model.forward_lowres(ops.resize_flip_image(x, s)) for s in ((32, 64), (64, 128), (96, 192))]
            assert all(low.shape[0] == 4 for low in lows)
            pred, cm = ops.multiscale_argmax_confusion(lows, [(False, True)] * 3, y, size=(64, 128), confusion=cm)
            preds.append(pred)
    assert torch.equal(ev.confusion, cm)                   # exactly the matrix of the hand-made calls
    want = E.confusion_metrics(cm.cpu().double())
    assert torch.equal(met['iou'], want['iou']) and met['miou'] == want['miou'] and met['accuracy'] == want['accuracy']
    assert set(met) == set(E.create_segmentation_evaluator(model, DEV).run(batches))          # the same metric dict
    valid = sum(int(((y >= 0) & (y < 19)).sum()) for _, y in batches)
    assert int(cm.sum()) == valid
    assert torch.equal(ev.predict(batches[0][0]), preds[0])
    again = ev.run(batches)
    assert torch.equal(ev.confusion, cm) and torch.equal(again['iou'], met['iou']) and torch.equal(again['dice'], met['dice'])

    plain = E.create_segmentation_evaluator(model, DEV)
    assert type(plain) is E.Evaluator


def test_multiscale_evaluator_needs_lowres_logits():
    from torch_semantic_segmentation_amd import engine as E
    with pytest.raises(NotImplementedError, match='forward_lowres'):
        E.MultiScaleEvaluator(torch.nn.Conv2d(3, 19, 1), DEV)


def test_launches_are_profiled_under_their_own_names():
    from torch_semantic_segmentation_amd import _native as N, ops
    (lows, flips), out = inputs('single', 19)
    x = torch.zeros(1, 3, 32, 64, device=DEV)
    N.prof_enable(True)
    try:
        N.prof_reset()
        ops.resize_flip_image(x, (16, 32))
        fused(lows, flips, out, torch.bfloat16, 'softmax')
        table = N.prof_table()
    finally:
        N.prof_enable(False)
        N.prof_reset()
    assert table['resize_flip_planar']['launches'] == 1 and table['multiscale_argmax_confusion']['launches'] == 1
    assert 'bilinear_planar_fwd' not in table and 'argmax_confusion' not in table      # not booked on the single-scale kernels
    assert table['multiscale_argmax_confusion']['symbol'] == 'multiscale_argmax_kernel'


def test_evaluator_options_and_empty_data():
    from torch_semantic_segmentation_amd import engine as E
    model = _model()
    ev = E.create_segmentation_evaluator(model, DEV, scales=(1.0,), flip=False, size_multiple=16, average='logits', ignore_index=7)
    assert (ev.size_multiple, ev.average, ev.ignore_index, ev.flip) == (16, 'logits', 7, False)
    assert ev.scaled_size(50, 75, 1.0) == (48, 80)
    with pytest.raises(ValueError, match='no batches'):
        ev.run([])
    with pytest.raises(ValueError, match='num_classes=5'):
        E.MultiScaleEvaluator(model, DEV, num_classes=5, scales=(1.0,), flip=False).predict(torch.zeros(1, 3, 64, 128))
