"""tss_classmix_select / tss_mix_batch (csrc/mix.hip) through the C ABI and the public wrappers, against the integer restatements of
tests/selftrain_ref.py.  Every comparison is bit for bit: the image is compared as integers (NaN and -0.0 payloads sit in the sources)."""
import numpy as np
import pytest
import torch

from tests import selftrain_ref as R
from tests.exact_gpu import DEV, N_

pytestmark = pytest.mark.gpu
DT = {'f32': torch.float32, 'bf16': torch.bfloat16}
ERR_SHAPE = -2
B, CI, H = 3, 3, 5
PARTNER = (1, 0, 2)                                         # sample 2 is its own partner


def images(W, dtype, seed=0):
    """[B][CI][H][W] random bit patterns of the dtype (every NaN payload, both zeros, denormals), with planted NaN / -0.0 / inf"""
    rng = np.random.default_rng(seed)
    if dtype == torch.float32:
        t = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (B, CI, H, W), dtype=np.int64).astype(np.int32)).view(torch.float32)
    else:
        t = torch.from_numpy(rng.integers(-2 ** 15, 2 ** 15, (B, CI, H, W), dtype=np.int64).astype(np.int16)).view(torch.bfloat16)
    t = t.clone()
    t[0, :, 0, :4] = float('nan')
    t[1, :, 0, :4] = -0.0
    t[1, :, 1, :4] = float('nan')
    t[0, :, 1, :4] = 0.0
    t[2, :, 2, :4] = float('-inf')
    return t


def label_maps(W, C, seed=1):
    """sample 0: no valid class (ignore bytes and bytes >= C); sample 1: one class; sample 2: five classes"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((B, H, W), dtype=np.uint8)
    lab[0] = rng.choice(np.array([255, C, 254], dtype=np.uint8), (H, W)) if C < 254 else 255
    lab[1] = C - 1
    lab[1, 0, :3] = 255
    lab[2] = rng.choice(np.array([0, 3, 7, C - 2, C - 1], dtype=np.uint8), (H, W))
    lab[2, 4, W - 1] = 255
    return lab


def key_rows(kind, C, seed=2):
    rng = np.random.default_rng(seed)
    if kind == 'random':
        return rng.integers(0, 2 ** 32, (B, 256), dtype=np.uint64).astype(np.uint32)
    if kind == 'equal':
        return np.full((B, 256), 77, dtype=np.uint32)
    k = np.full((B, 256), 5, dtype=np.uint32)            # 'topbit': keys that differ in the top bit only
    k[:, [0, 7, C - 1]] |= np.uint32(0x80000000)
    return k


def select(lab, keys, C):
    n = N_()
    labd = torch.from_numpy(lab).to(DEV)
    keyd = torch.from_numpy(keys.view(np.int32)).to(DEV)
    sel = torch.full((B + 1, 256), 9, dtype=torch.uint8, device=DEV)
    n.call('tss_classmix_select', labd.data_ptr(), keyd.data_ptr(), sel.data_ptr(), B, lab[0].size, C, n.stream())
    torch.cuda.synchronize()
    assert (sel[B] == 9).all(), 'a row behind sel written'
    return sel[:B].contiguous()


def mix(img, lab, partner, sel=None, boxes=None):
    """the C entry with NaN / -1 filled outputs and guard elements behind them; returns (image bits, target)"""
    n = N_()
    imgd, labd = img.to(DEV), torch.from_numpy(lab).to(DEV)
    pd = torch.tensor(partner, dtype=torch.int32, device=DEV)
    bd = torch.tensor(boxes, dtype=torch.int32, device=DEV) if boxes is not None else None
    numel = img.numel()
    out = torch.full((numel + 64,), float('nan'), dtype=img.dtype, device=DEV)
    out[numel:] = 7.25
    tgt = torch.full((lab.size + 16,), -1, dtype=torch.int64, device=DEV)
    W = img.shape[3]
    n.call('tss_mix_batch', imgd.data_ptr(), labd.data_ptr(), pd.data_ptr(), n.ptr(sel), n.ptr(bd), out.data_ptr(), tgt.data_ptr(), B, CI, H, W,
           n.dtype_code(img.dtype), n.stream())
    torch.cuda.synchronize()
    assert (out[numel:].float() == 7.25).all() and (tgt[lab.size:] == -1).all(), 'elements behind an output written'
    return R.bits_of(out[:numel].reshape(img.shape)), tgt[:lab.size].reshape(lab.shape).cpu().numpy()


@pytest.mark.parametrize('d', ['f32', 'bf16'])
@pytest.mark.parametrize('W', [24, 264])
def test_boxes(W, d):
    img, lab = images(W, DT[d]), label_maps(W, 19)
    rows = [[(0, 0, 0, 0), (0, 0, H, W), (2, 3, 4, 14)],                  # empty; the whole image; columns 3..13, no multiple of 8
            [(0, 0, 2, W), (H - 2, 0, H, W), (0, 0, H, 5)],                # touching the top, the bottom, the left edge
            [(1, W - 7, H, W), (3, 5, 3, 9), (0, W - 1, 1, W)],            # the right edge; y0 == y1; the last pixel of the first row
            [(0, 3, H, 14), (2, 8, 3, 16), (4, 0, 5, 1)]]                  # whole columns 3..13; one aligned group; the first pixel of the last row
    if W > 256:
        rows.append([(0, 250, H, 262), (1, 255, 2, 257), (0, 256, H, W)])  # across and at the 256-lane boundary
    for boxes in rows:
        got_i, got_t = mix(img, lab, PARTNER, boxes=boxes)
        want_i, want_t = R.mix_batch(R.bits_of(img), lab, PARTNER, boxes=np.array(boxes))
        assert np.array_equal(got_i, want_i), (W, d, boxes, 'image bits')
        assert np.array_equal(got_t, want_t), (W, d, boxes, 'target')
    assert np.isnan(img[0, :, 0, :4].float().numpy()).all() and rows[0][0] == (0, 0, 0, 0)   # the NaN of sample 0 was NOT chosen there ...
    got_i, _ = mix(img, lab, PARTNER, boxes=rows[0])
    assert np.array_equal(got_i[0], R.bits_of(img)[1])                                        # ... and did not reach the output


@pytest.mark.parametrize('d', ['f32', 'bf16'])
@pytest.mark.parametrize('W', [24, 264])
@pytest.mark.parametrize('C', [19, 66])
@pytest.mark.parametrize('kind', ['random', 'equal', 'topbit'])
def test_class_picks(kind, C, W, d):
    img, lab, keys = images(W, DT[d]), label_maps(W, C), key_rows(kind, C)
    sel = select(lab, keys, C)
    want_sel = R.classmix_select(lab, keys, C)
    assert np.array_equal(sel.cpu().numpy(), want_sel), (kind, C, 'sel')
    assert want_sel[0].sum() == 0 and want_sel[1].sum() == 1 and want_sel[1, C - 1] == 1 and want_sel[2].sum() == 3
    if kind == 'equal':
        assert np.nonzero(want_sel[2])[0].tolist() == [0, 3, 7]                              # ties: the lower class indices
    if kind == 'topbit':
        assert np.nonzero(want_sel[2])[0].tolist() == [0, 3, C - 2]                         # 3, C - 2 (top bit clear), then 0 by index
        assert want_sel[2, 7] == 0 and want_sel[2, C - 1] == 0                               # a set top bit ranks above a clear one
    got_i, got_t = mix(img, lab, PARTNER, sel=sel)
    want_i, want_t = R.mix_batch(R.bits_of(img), lab, PARTNER, sel=want_sel)
    assert np.array_equal(got_i, want_i), (kind, C, W, d, 'image bits')
    assert np.array_equal(got_t, want_t) and got_t.dtype == np.int64, (kind, C, W, d, 'target')
    assert (got_t[0] == lab[1]).all() and (got_t == 255).any()                               # no class picked: the partner's map; 255 stays


def test_select_unaligned_and_short_maps():
    """maps whose length is no multiple of 16 and whose rows do not start on 16 bytes (the head / vector / tail split of the reader)"""
    n = N_()
    rng = np.random.default_rng(5)
    for HW in (1, 15, 16, 17, 1000, 40 * 1024 + 3):
        lab = rng.integers(0, 256, (B, HW)).astype(np.uint8)
        lab[1] = 200                                      # one class (of 256) or none (of 19)
        keys = key_rows('random', 19, seed=HW)
        for C in (19, 256):
            labd = torch.from_numpy(lab).to(DEV)
            keyd = torch.from_numpy(keys.view(np.int32)).to(DEV)
            sel = torch.empty((B, 256), dtype=torch.uint8, device=DEV)
            n.call('tss_classmix_select', labd.data_ptr(), keyd.data_ptr(), sel.data_ptr(), B, HW, C, n.stream())
            torch.cuda.synchronize()
            assert np.array_equal(sel.cpu().numpy(), R.classmix_select(lab, keys, C)), (HW, C)


def test_argument_errors():
    n = N_()
    lib = n.lib()
    img, lab = images(24, torch.float32).to(DEV), torch.from_numpy(label_maps(24, 19)).to(DEV)
    out, tgt = torch.zeros_like(img), torch.zeros((B, H, 24), dtype=torch.int64, device=DEV)
    pd = torch.tensor(PARTNER, dtype=torch.int32, device=DEV)
    sel = torch.zeros((B, 256), dtype=torch.uint8, device=DEV)
    bx = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()

    def rc(s, b, W=24):
        return lib.tss_mix_batch(p(img), p(lab), p(pd), p(s), p(b), p(out), p(tgt), B, CI, H, W, 0, n.stream())

    assert rc(sel, bx) == ERR_SHAPE and rc(None, None) == ERR_SHAPE        # both, neither
    assert rc(None, bx, W=20) == ERR_SHAPE and rc(sel, None, W=12) == ERR_SHAPE
    assert rc(None, bx) == 0 and rc(sel, None) == 0
    assert lib.tss_mix_batch(p(img), p(lab), p(pd), None, p(bx), p(out), p(tgt), B, CI, H, 24, 7, n.stream()) == -1     # dtype
    torch.cuda.synchronize()


def test_public_wrappers():
    import torch_semantic_segmentation_amd as tssa
    W, C = 24, 19
    img, lab, keys = images(W, torch.float32), label_maps(W, C), key_rows('random', C)
    labd = torch.from_numpy(lab).to(DEV)
    sel = tssa.classmix_select(labd, keys, C)                              # host keys: validated and copied
    assert np.array_equal(sel.cpu().numpy(), R.classmix_select(lab, keys, C))
    sel_d = tssa.classmix_select(labd, torch.from_numpy(keys.view(np.int32)).to(DEV), C)      # device keys: as they are
    assert torch.equal(sel, sel_d)
    oi, ot = tssa.mix_batch(img.to(DEV), labd, list(PARTNER), sel=sel)
    wi, wt = R.mix_batch(R.bits_of(img), lab, PARTNER, sel=R.classmix_select(lab, keys, C))
    assert np.array_equal(R.bits_of(oi), wi) and np.array_equal(ot.cpu().numpy(), wt)
    boxes = [(0, 0, 2, 8), (1, 3, 4, 14), (0, 0, H, W)]
    out_i, out_t = torch.empty_like(img, device=DEV), torch.empty((B, H, W), dtype=torch.int64, device=DEV)
    oi, ot = tssa.mix_batch(img.to(DEV), labd, np.array(PARTNER), boxes=boxes, out_image=out_i, out_target=out_t)
    wi, wt = R.mix_batch(R.bits_of(img), lab, PARTNER, boxes=np.array(boxes))
    assert oi is out_i and ot is out_t and np.array_equal(R.bits_of(oi), wi) and np.array_equal(ot.cpu().numpy(), wt)
    for bad in (dict(partner=[0, 1, 3], boxes=boxes), dict(partner=[0, 1], boxes=boxes), dict(partner=[0.5, 1, 2], boxes=boxes),
                dict(partner=PARTNER, boxes=[(0, 0, H + 1, W)] * 3), dict(partner=PARTNER, boxes=[(0, 0, H, W + 1)] * 3),
                dict(partner=PARTNER, boxes=[(0, -1, H, W)] * 3), dict(partner=PARTNER), dict(partner=PARTNER, sel=sel, boxes=boxes)):
        with pytest.raises(ValueError):
            tssa.mix_batch(img.to(DEV), labd, **bad)
    with pytest.raises(ValueError):
        tssa.mix_batch(img[..., :20].contiguous().to(DEV), labd[..., :20].contiguous(), PARTNER, boxes=boxes)
    with pytest.raises(ValueError):
        tssa.classmix_select(labd, keys[:2], C)
    with pytest.raises(ValueError):
        tssa.classmix_select(labd, keys.astype(np.int64) + 2 ** 32, C)
