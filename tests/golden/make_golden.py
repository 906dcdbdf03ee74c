#!/usr/bin/env python
"""Generate tests/golden/*.npz by running the REFERENCE itself (imported from /root/reference, CPU).

Run in the build container only:   python tests/golden/make_golden.py
The reference's Python never travels; only the arrays written here do.  Weights and inputs are
closed-form (oracle/recipe.py: formula_state, lattice_input, lattice_target), so each fixture stores
outputs only.  Dropout is forced to p=0 for train-mode fixtures (CPU mt19937 masks are not
reproducible on a GPU; SURVEY.md §7 "hard parts").

Fixture families:
  G1 blocks_*.npz : per-block forward / dX / dW for every block type of rows A-H and K-P
  G2 eval_*.npz   : whole-model eval logits (pre-upsample, strided full-res sample) + argmax mask
  G3 train_*.npz  : 2 train steps (CE(ignore 255) + AdamW): loss, per-parameter grad norms, a few
                    full gradients, BN running stats, post-step parameter norms.  NOTE: whole-model
                    train-mode gradients of these networks are ill-conditioned in f32 (the reference's own
                    f32 and f64 gradients differ by 2-130%), so the tests use the
                    losses and running statistics from this file and compare gradients against an f64
                    run of the oracle instead.
  G3c train_seeded.npz: ONE train-mode forward/backward with default init (torch.manual_seed(0)) on the seeded N(0,1)
                    batch at 2x3x96x160, by the reference in f32 AND in f64: the conditioning yardstick err_ref32 and
                    the f64 gradients the GPU train-mode gradient test is held to (3 x err_ref32)
  G3b frozen_*.npz: the same two steps with BatchNorm frozen (model.eval(): running statistics,
                    Dropout off) -- a well-conditioned end-to-end backward (f32 vs f64 differ by 1e-6):
                    loss, ALL per-parameter grad norms, full gradients of representative tensors
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, '/root/reference')

from oracle.recipe import formula_state, lattice_input, lattice_target, train_step  # noqa: E402
import importlib                                                                  # noqa: E402
ref_fast = importlib.import_module('torch_semantic_segmentation.models.fastscnn')
ref_ctx = importlib.import_module('torch_semantic_segmentation.models.contextnet')

torch.set_num_threads(4)
torch.use_deterministic_algorithms(True)


def zero_dropout(m):
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0


def np32(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------- G1: blocks

def block_cases():
    """name -> (constructor thunk, input shapes).  Shapes are (B,C,H,W); two inputs for fusion."""
    f, c = ref_fast, ref_ctx
    return {
        # FastSCNN rows A-H
        'fast_stem':        (lambda: f.Conv2dBlock(3, 32, kernel_size=3, padding=1, stride=2), [(2, 3, 16, 32)]),
        'fast_pw_act':      (lambda: f.Conv2dBlock(48, 96, kernel_size=1), [(2, 48, 8, 16)]),
        'fast_pw_noact':    (lambda: f.Conv2dBlock(64, 32, kernel_size=1, use_activation=False), [(2, 64, 8, 16)]),
        'fast_dw_s1':       (lambda: f.DWConv2dBlock(48, 48, kernel_size=3, padding=1), [(2, 48, 8, 16)]),
        'fast_dw_s2':       (lambda: f.DWConv2dBlock(32, 32, kernel_size=3, padding=1, stride=2), [(2, 32, 8, 16)]),
        'fast_dw_d4':       (lambda: f.DWConv2dBlock(32, 32, kernel_size=3, padding=4, dilation=4), [(2, 32, 8, 16)]),
        'fast_ds_s2':       (lambda: f.DSConv2dBlock(32, 48, kernel_size=3, padding=1, stride=2), [(2, 32, 8, 16)]),
        'fast_ds_s1':       (lambda: f.DSConv2dBlock(32, 32, kernel_size=3, padding=1), [(2, 32, 8, 16)]),
        'fast_bneck_res':   (lambda: f.BottleneckBlock(32, 32, expansion=6), [(2, 32, 8, 16)]),
        'fast_bneck_s2':    (lambda: f.BottleneckBlock(32, 48, stride=2, expansion=6), [(2, 32, 8, 16)]),
        'fast_bneck_mod':   (lambda: f.BottleneckModule(32, 48, expansion=6, repeats=3, stride=2), [(2, 32, 8, 16)]),
        'fast_ppm':         (lambda: f.PyramidPoolingModule(64, 64), [(2, 64, 8, 16)]),
        'fast_ppm_odd':     (lambda: f.PyramidPoolingModule(32, 32), [(3, 32, 8, 20)]),
        'fast_fusion':      (lambda: f.FeatureFusionModule((48, 32), 64, scale_factor=4), [(2, 48, 2, 4), (2, 32, 8, 16)]),
        'fast_classifier':  (lambda: f.Classifier(32, 19), [(2, 32, 8, 16)]),
        # ContextNet rows K-P
        'ctx_stem':         (lambda: c.ConvBlock(3, 32, 3, padding=1, stride=2), [(2, 3, 16, 32)]),
        'ctx_dense3x3':     (lambda: c.ConvBlock(32, 32, 3, padding=1), [(2, 32, 8, 16)]),
        'ctx_pw':           (lambda: c.ConvBlock(32, 64, 1), [(2, 32, 8, 16)]),
        'ctx_dw_s2':        (lambda: c.DWConvBlock(64, 64, kernel_size=3, padding=1, stride=2), [(2, 64, 8, 16)]),
        'ctx_bneck_e1':     (lambda: c.BottleneckBlock(32, 32, expansion=1), [(2, 32, 8, 16)]),
        'ctx_bneck_e6':     (lambda: c.BottleneckBlock(32, 32, expansion=6), [(2, 32, 8, 16)]),
        'ctx_linear_bneck': (lambda: c.LinearBottleneck(32, 48, 3, stride=2), [(2, 32, 8, 16)]),
        'ctx_fusion':       (lambda: c.FeatureFusionModule((48, 32), 64), [(2, 48, 2, 4), (2, 32, 8, 16)]),
        'ctx_classifier':   (lambda: c.Classifier(32, 19), [(2, 32, 8, 16)]),
    }


def run_block(make, shapes, training):
    m = make()
    m.load_state_dict(formula_state(m), strict=True)
    zero_dropout(m)
    m.train(training)
    xs = [lattice_input(*s).mul(1.0 + 0.25 * i).requires_grad_(True) for i, s in enumerate(shapes)]
    out = m(*xs)
    # a fixed, non-trivial cotangent
    cot = lattice_input(*out.shape).flip(1) * 0.5 + 0.1
    out.backward(cot)
    rec = {'out': np32(out)}
    for i, x in enumerate(xs):
        rec['dx%d' % i] = np32(x.grad)
    for name, p in m.named_parameters():
        rec['dw.' + name] = np32(p.grad)
    if training:
        for name, b in m.named_buffers():
            if name.endswith('running_mean') or name.endswith('running_var'):
                rec['buf.' + name] = np32(b)
    return rec


def gen_blocks():
    for mode in ('train', 'eval'):
        blob = {}
        for name, (make, shapes) in block_cases().items():
            rec = run_block(make, shapes, training=(mode == 'train'))
            for k, v in rec.items():
                blob['%s/%s' % (name, k)] = v
        path = os.path.join(HERE, 'blocks_%s.npz' % mode)
        np.savez_compressed(path, **blob)
        print('wrote', path, '%.1f KiB' % (os.path.getsize(path) / 1024), len(blob), 'arrays')


# ----------------------------------------------------------------------------- G2: whole-model eval

MODELS = {
    'fastscnn': lambda: ref_fast.fastscnn(3, 19),
    'contextnet12': lambda: ref_ctx.contextnet12(3, 19),
    'contextnet14': lambda: ref_ctx.contextnet14(3, 19),
    'contextnet18': lambda: ref_ctx.contextnet18(3, 19),
}
EVAL_SHAPE = (2, 3, 64, 128)


def gen_eval():
    blob = {}
    for name, make in MODELS.items():
        m = make()
        m.load_state_dict(formula_state(m, gain=1.0), strict=True)
        m.eval()
        low = {}
        h = m.classifier.register_forward_hook(lambda _m, _i, o: low.__setitem__('v', o))
        with torch.no_grad():
            logits = m(lattice_input(*EVAL_SHAPE))
        h.remove()
        top2 = logits.topk(2, dim=1).values
        blob[name + '/low'] = np32(low['v'])
        blob[name + '/sub'] = np32(logits[:, :, ::4, ::4])
        blob[name + '/argmax'] = logits.argmax(1).to(torch.uint8).numpy()
        blob[name + '/gap'] = np32(top2[:, 0] - top2[:, 1])
        blob[name + '/sum_abs'] = np.array([logits.sum().item(), logits.abs().sum().item()])
        print(name, 'logit range', logits.min().item(), logits.max().item(),
              'min top-2 gap', (top2[:, 0] - top2[:, 1]).min().item())
    path = os.path.join(HERE, 'eval_models.npz')
    np.savez_compressed(path, **blob)
    print('wrote', path, '%.1f KiB' % (os.path.getsize(path) / 1024))


# ----------------------------------------------------------------------------- G3: train steps

TRAIN_SHAPE = (2, 3, 64, 128)
FULL_GRADS = {
    'fastscnn': ['downsample.0.0.weight', 'downsample.1.0.weight', 'features.0.0.conv1.0.weight',
                 'features.0.1.conv2.1.weight', 'features.3.conv.0.weight', 'fusion.lowres.1.0.weight',
                 'classifier.3.weight', 'classifier.3.bias'],
    'contextnet14': ['spatial.0.0.weight', 'spatial.1.0.weight', 'context.7.0.weight',
                     'context.3.0.conv2.1.bias', 'feature_fusion.highres.0.weight',
                     'classifier.5.weight', 'classifier.5.bias'],
}


def gen_train():
    blob = {}
    for name in ('fastscnn', 'contextnet14'):
        m = MODELS[name]()
        m.load_state_dict(formula_state(m), strict=True)
        zero_dropout(m)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
        loss_fn = nn.CrossEntropyLoss(ignore_index=255)
        x = lattice_input(*TRAIN_SHAPE)
        y = lattice_target(TRAIN_SHAPE[0], TRAIN_SHAPE[2], TRAIN_SHAPE[3])
        losses = []
        for step in range(2):
            losses.append(train_step(m, opt, loss_fn, x, y))
            if step == 0:
                names = [n for n, _ in m.named_parameters()]
                blob[name + '/grad_norms'] = np.array(
                    [p.grad.double().norm().item() for _, p in m.named_parameters()])
                for n in FULL_GRADS[name]:
                    blob[name + '/grad.' + n] = np32(m.get_parameter(n).grad)
                blob[name + '/param_norms_after1'] = np.array(
                    [p.detach().double().norm().item() for _, p in m.named_parameters()])
                for n, b in m.named_buffers():
                    if n.endswith('running_mean') or n.endswith('running_var'):
                        blob[name + '/buf_norm.' + n] = np.array(b.double().norm().item())
                assert names == [n for n, _ in m.named_parameters()]
        blob[name + '/losses'] = np.array(losses)
        blob[name + '/param_norms_after2'] = np.array(
            [p.detach().double().norm().item() for _, p in m.named_parameters()])
        print(name, 'losses', losses)
    path = os.path.join(HERE, 'train_steps.npz')
    np.savez_compressed(path, **blob)
    print('wrote', path, '%.1f KiB' % (os.path.getsize(path) / 1024))


def frozen_step(m, opt, loss_fn, x, y):
    """update_fn with the model kept in eval mode (frozen BatchNorm fine-tuning)."""
    m.eval()
    opt.zero_grad()
    loss = loss_fn(m(x), y)
    loss.backward()
    opt.step()
    return loss.item()


def gen_frozen():
    blob = {}
    for name in ('fastscnn', 'contextnet12', 'contextnet14', 'contextnet18'):
        m = MODELS[name]()
        m.load_state_dict(formula_state(m), strict=True)
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
        loss_fn = nn.CrossEntropyLoss(ignore_index=255)
        x = lattice_input(*TRAIN_SHAPE)
        y = lattice_target(TRAIN_SHAPE[0], TRAIN_SHAPE[2], TRAIN_SHAPE[3])
        losses = [frozen_step(m, opt, loss_fn, x, y)]
        blob[name + '/grad_norms'] = np.array([p.grad.double().norm().item() for _, p in m.named_parameters()])
        for n in FULL_GRADS.get(name, FULL_GRADS['contextnet14']):
            blob[name + '/grad.' + n] = np32(m.get_parameter(n).grad)
        losses.append(frozen_step(m, opt, loss_fn, x, y))
        blob[name + '/losses'] = np.array(losses)
        blob[name + '/param_norms_after2'] = np.array(
            [p.detach().double().norm().item() for _, p in m.named_parameters()])
        print(name, 'frozen losses', losses)
    path = os.path.join(HERE, 'frozen_steps.npz')
    np.savez_compressed(path, **blob)
    print('wrote', path, '%.1f KiB' % (os.path.getsize(path) / 1024))


# ----------------------------------------------------------------------------- G5: PSPNet head

def pspnet_cases():
    ref_psp = importlib.import_module('torch_semantic_segmentation.models.pspnet')
    ref_led = importlib.import_module('torch_semantic_segmentation.models.lednet')
    return {
        'psp_ppm': (lambda: ref_psp.PyramidPoolingModule(64, 64, pools=[1, 2, 3, 6]), [(2, 64, 12, 20)]),
        'psp_net': (lambda: ref_psp.PSPNet(nn.Identity(), 19, 64), [(2, 64, 12, 20)]),
        'psp_ppm_odd': (lambda: ref_psp.PyramidPoolingModule(32, 64, pools=[1, 2, 3, 6]), [(3, 32, 9, 14)]),
        # LEDNet split-shuffle-non-bottleneck unit (TSS/models/lednet.py:95-124), dilations of the encoder's stages
        'led_ssnbt_d1': (lambda: ref_led.SSnbtBlock(64, 64, dilation=1), [(2, 64, 12, 20)]),
        'led_ssnbt_d5': (lambda: ref_led.SSnbtBlock(128, 128, dilation=5), [(2, 128, 12, 20)]),
        'led_ssnbt_d9': (lambda: ref_led.SSnbtBlock(32, 32, dilation=9), [(2, 32, 24, 10)]),
        # BiSeNet's attention blocks (TSS/models/bisenet.py:112-148)
        'bise_arm': (lambda: importlib.import_module('torch_semantic_segmentation.models.bisenet').AttentionRefinementModule(64, 64),
                     [(2, 64, 12, 20)]),
        'bise_ffm': (lambda: importlib.import_module('torch_semantic_segmentation.models.bisenet').FeatureFusionModule(96, 64),
                     [(2, 96, 12, 20)]),
    }


def gen_pspnet():
    blob = {}
    for mode in ('train', 'eval'):
        for name, (make, shapes) in pspnet_cases().items():
            rec = run_block(make, shapes, training=(mode == 'train'))
            for k, v in rec.items():
                blob['%s/%s/%s' % (mode, name, k)] = v
    path = os.path.join(HERE, 'pspnet.npz')
    np.savez_compressed(path, **blob)
    print('wrote', path, '%.1f KiB' % (os.path.getsize(path) / 1024), len(blob), 'arrays')


# ----------------------------------------------------------------------------- G6: LEDNet + ESNet blocks

def zoo_cases():
    led = importlib.import_module('torch_semantic_segmentation.models.lednet')
    es = importlib.import_module('torch_semantic_segmentation.models.esnet')
    return {
        # LEDNet (TSS/models/lednet.py): encoder down-sampler on the image and on an activation, the APN decoder with 19 classes
        'led_down_img': (lambda: led.DownsamplingBlock(3, 32), [(2, 3, 16, 24)]),
        'led_down': (lambda: led.DownsamplingBlock(32, 64), [(2, 32, 12, 20)]),
        'led_apn': (lambda: led.APNModule(32, 19), [(2, 32, 16, 24)]),
        # ESNet (TSS/models/esnet.py): factorized units with K = 3 and K = 5, the parallel dilated unit, the down-sampler 16 -> 64
        'es_fcu3': (lambda: es.FCUBlock(16, 16, 3), [(2, 16, 12, 20)]),
        'es_fcu5': (lambda: es.FCUBlock(32, 32, 5), [(2, 32, 12, 20)]),
        'es_fpcu': (lambda: es.FPCUBlock(32, 32, [2, 5, 9]), [(2, 32, 12, 20)]),
        'es_down': (lambda: es.DownsamplingBlock(16, 64), [(2, 16, 12, 20)]),
        'es_up': (lambda: es.UpsamplingBlock(64, 16), [(2, 64, 6, 10)]),
        'es_up_cls': (lambda: es.UpsamplingBlock(16, 19), [(2, 16, 6, 10)]),
    }


def zero_all_dropout(m):
    for mod in m.modules():
        if isinstance(mod, (nn.Dropout, nn.Dropout2d)):
            mod.p = 0.0


def gen_zoo():
    """Blocks: forward, dX and every parameter gradient in train and eval mode (formula weights, lattice input, fixed cotangent).
    Whole LedNet (TSS/models/lednet.py:13-55) on a 2 x 3 x 64 x 128 lattice image: eval-mode logits (every 4th pixel, f32) and
    the full arg-max map; train-mode logits of the same (dropout p = 0: torch's Dropout2d draws cannot be reproduced elsewhere).
    Whole ESNet (TSS/models/esnet.py:8-44) on a 2 x 3 x 32 x 64 lattice image, the same way."""
    blob = {}
    for mode in ('train', 'eval'):
        for name, (make, shapes) in zoo_cases().items():
            def make0(make=make):
                m = make()
                zero_all_dropout(m)
                return m
            rec = run_block(make0, shapes, training=(mode == 'train'))
            for k, v in rec.items():
                blob['%s/%s/%s' % (mode, name, k)] = v
    led = importlib.import_module('torch_semantic_segmentation.models.lednet')
    m = led.lednet(3, 19)
    m.load_state_dict(formula_state(m), strict=True)
    zero_all_dropout(m)
    x = lattice_input(2, 3, 64, 128)
    m.eval()
    with torch.no_grad():
        out = m(x)
    blob['eval/led_net/out_sub4'] = np32(out[:, :, ::4, ::4])
    blob['eval/led_net/argmax'] = out.argmax(1).numpy().astype(np.uint8)
    blob['eval/led_net/lowres'] = np32(m.decoder(m.encoder(x)))
    m.train()
    out = m(x)
    blob['train/led_net/out_sub4'] = np32(out[:, :, ::4, ::4].detach())
    for n, b in m.named_buffers():
        if n.endswith('running_mean') or n.endswith('running_var'):
            blob['train/led_net/buf_norm.' + n] = np.array(b.double().norm().item())
    es = importlib.import_module('torch_semantic_segmentation.models.esnet')
    m = es.ESNet(3, 19)
    m.load_state_dict(formula_state(m), strict=True)
    zero_all_dropout(m)
    x = lattice_input(2, 3, 32, 64)
    m.eval()
    with torch.no_grad():
        out = m(x)
    blob['eval/es_net/out_sub2'] = np32(out[:, :, ::2, ::2])
    blob['eval/es_net/argmax'] = out.argmax(1).numpy().astype(np.uint8)
    m.train()
    out = m(x)
    blob['train/es_net/out_sub2'] = np32(out[:, :, ::2, ::2].detach())
    # the train-mode forward of this fixture is ill-conditioned (tiny maps, ReLU / max-pool decisions on near-ties): the reference in
    # f64 is the anchor and its own f32 distance from it the yardstick (as for the whole-model gradients of G3c)
    m64 = es.ESNet(3, 19)
    m64.load_state_dict(formula_state(m64), strict=True)
    zero_all_dropout(m64)
    m64.double().train()
    out64 = m64(x.double()).detach()
    blob['train/es_net/out64_sub2'] = out64[:, :, ::2, ::2].numpy()
    blob['train/es_net/err_ref32'] = np.array(((out.detach().double() - out64).abs().max() / out64.abs().max()).item())
    print('es_net train err_ref32', blob['train/es_net/err_ref32'])
    path = os.path.join(HERE, 'zoo.npz')
    np.savez_compressed(path, **blob)
    print('wrote', path, '%.1f KiB' % (os.path.getsize(path) / 1024), len(blob), 'arrays')


def gen_zoo_frozen():
    """G5b (round 4): whole LedNet / ESNet, one backward pass with the BatchNorms frozen -- default init under torch.manual_seed(0) (the
    closed-form weights make ESNet's gradient differ by 35 % between the reference's own f32 and f64 runs), the seeded N(0,1) batch at
    2 x 3 x 64 x 128, Dropout p = 0, running statistics that fit the weights (one train-mode forward with momentum 1 in f64, stored
    as f32).  Even so these 40-layer ReLU / max-pool stacks are ill-conditioned at this size: the reference's f32 gradients are 0.5 - 4 %
    from its f64 ones, tensor by tensor.  So, as for G3c: the f64 run is the anchor and the reference's own f32 distance, per tensor, the
    yardstick (x 3 in the GPU test).  Stored: both losses, per-parameter weight checksums (the tests rebuild the weights from the seed),
    the buffers, gradient norms of both runs, err_ref32 per tensor, full f64 gradients of five representative tensors."""
    from oracle.recipe import synthetic_batch
    blob = {}
    led = importlib.import_module('torch_semantic_segmentation.models.lednet')
    es = importlib.import_module('torch_semantic_segmentation.models.esnet')
    shape = (2, 64, 128)
    x, y = synthetic_batch(*shape)
    for name, make in (('led_net', lambda: led.lednet(3, 19)), ('es_net', lambda: es.ESNet(3, 19))):
        def build(dt):
            torch.manual_seed(0)
            m = make()
            zero_all_dropout(m)
            return m.to(dt)
        # running statistics: batch statistics of the f64 network, rounded to f32 (both runs then use the SAME numbers)
        m64 = build(torch.float64)
        moms = [(b, b.momentum) for b in m64.modules() if isinstance(b, nn.BatchNorm2d)]
        for b, _ in moms:
            b.momentum = 1.0
        m64.train()
        with torch.no_grad():
            m64(x.double())
        for b, mo in moms:
            b.momentum = mo
        bufs = {n: b.detach().float() for n, b in m64.named_buffers() if n.endswith('running_mean') or n.endswith('running_var')}
        runs = {}
        for dt in (torch.float32, torch.float64):
            m = build(dt)
            with torch.no_grad():
                for n, b in m.named_buffers():
                    if n in bufs:
                        b.copy_(bufs[n].to(dt))
            m.eval()
            loss = nn.CrossEntropyLoss(ignore_index=255)(m(x.to(dt)), y)
            loss.backward()
            runs[dt] = (m, loss.item())
        (m32, l32), (m64, l64) = runs[torch.float32], runs[torch.float64]
        for n, v in bufs.items():
            blob[name + '/buf.' + n] = np32(v)
        blob[name + '/loss32'] = np.array(l32)
        blob[name + '/loss64'] = np.array(l64)
        blob[name + '/wsum'] = np.array([p.detach().double().abs().sum().item() for p in m32.parameters()])
        blob[name + '/grad_norms32'] = np.array([p.grad.double().norm().item() for p in m32.parameters()])
        blob[name + '/grad_norms64'] = np.array([p.grad.norm().item() for p in m64.parameters()])
        blob[name + '/err_ref32_per_tensor'] = np.array(
            [((p.grad.double() - q.grad).norm() / q.grad.norm().clamp_min(1e-300)).item() for p, q in zip(m32.parameters(), m64.parameters())])
        convs = [n for n, p in m64.named_parameters() if p.dim() == 4]
        for n in (convs[0], convs[len(convs) // 3], convs[len(convs) // 2], convs[-2], convs[-1]):
            blob[name + '/grad64.' + n] = m64.get_parameter(n).grad.numpy()
        e = blob[name + '/err_ref32_per_tensor']
        print(name, 'loss32', l32, 'loss64', l64, 'err_ref32 per tensor: median %.2e max %.2e' % (np.median(e), e.max()))
    path = os.path.join(HERE, 'zoo_frozen.npz')
    np.savez_compressed(path, **blob)
    print('wrote', path, '%.1f KiB' % (os.path.getsize(path) / 1024), len(blob), 'arrays')


# ----------------------------------------------------------------------------- G3c: train step, default init, f32 AND f64

SEEDED_SHAPE = (2, 96, 160)


def gen_seeded():
    """The well-conditioned whole-model train-mode gradient fixture: torch.manual_seed(0) default init (the reference has
    no custom init), the seeded N(0,1) batch of SURVEY.md section 8d at 2 x 3 x 96 x 160, Dropout p = 0.  The reference runs
    once in f32 and once in f64 (model.double()): err_ref32 = |g32 - g64| / |g64| over ALL parameters is the yardstick
    the GPU test multiplies by 3 (it is ~1e-3 here, against 0.9-1.3 on the closed-form-weight fixture G3)."""
    from oracle.recipe import synthetic_batch
    blob = {}
    for name in ('fastscnn', 'contextnet14'):
        x, y = synthetic_batch(*SEEDED_SHAPE)
        loss_fn = nn.CrossEntropyLoss(ignore_index=255)
        runs = {}
        for dt in (torch.float32, torch.float64):
            torch.manual_seed(0)
            m = MODELS[name]()
            zero_dropout(m)
            m.to(dt).train()
            out = m(x.to(dt))
            loss = loss_fn(out, y)
            loss.backward()
            runs[dt] = (m, out.detach(), loss.item())
        (m32, o32, l32), (m64, o64, l64) = runs[torch.float32], runs[torch.float64]
        g32 = torch.cat([p.grad.flatten().double() for p in m32.parameters()])
        g64 = torch.cat([p.grad.flatten() for p in m64.parameters()])
        blob[name + '/loss32'] = np.array(l32)
        blob[name + '/loss64'] = np.array(l64)
        blob[name + '/err_ref32'] = np.array(((g32 - g64).norm() / g64.norm()).item())
        blob[name + '/err_logits_ref32'] = np.array(((o32.double() - o64).abs().max() / o64.abs().max()).item())
        blob[name + '/grad_norms32'] = np.array([p.grad.double().norm().item() for p in m32.parameters()])
        blob[name + '/grad_norms64'] = np.array([p.grad.norm().item() for p in m64.parameters()])
        blob[name + '/err_ref32_per_tensor'] = np.array(
            [((p.grad.double() - q.grad).norm() / q.grad.norm().clamp_min(1e-300)).item()
             for p, q in zip(m32.parameters(), m64.parameters())])
        blob[name + '/logits64_sub'] = o64[:, :, ::8, ::8].numpy()
        for n in FULL_GRADS[name]:
            blob[name + '/grad64.' + n] = m64.get_parameter(n).grad.numpy()
        for n, b in m64.named_buffers():
            if n.endswith('running_mean') or n.endswith('running_var'):
                blob[name + '/buf_norm64.' + n] = np.array(b.norm().item())
        print(name, 'loss32', l32, 'loss64', l64, 'err_ref32', blob[name + '/err_ref32'], 'logits', blob[name + '/err_logits_ref32'])
    path = os.path.join(HERE, 'train_seeded.npz')
    np.savez_compressed(path, **blob)
    print('wrote', path, '%.1f KiB' % (os.path.getsize(path) / 1024))


# ----------------------------------------------------------------------------- state_dict layout of the reference models

def gen_keys():
    """The reference's state_dict layout (key order, shapes, dtypes) of FastSCNN and ContextNet12, as strings: the oracle's
    key / shape contract is checked against it without importing the reference."""
    blob = {}
    for name, m in (('fastscnn', ref_fast.fastscnn(3, 19)), ('contextnet12', ref_ctx.contextnet12(3, 19))):
        sd = m.state_dict()
        blob[name + '/keys'] = np.array(list(sd))
        blob[name + '/shapes'] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
        blob[name + '/dtypes'] = np.array([str(v.dtype) for v in sd.values()])
    path = os.path.join(HERE, 'state_dict_keys.npz')
    np.savez_compressed(path, **blob)
    print('wrote', path, '%.1f KiB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    which = sys.argv[1:] or ['blocks', 'eval', 'train', 'frozen', 'seeded', 'pspnet', 'zoo', 'zoo_frozen', 'keys']
    if 'keys' in which:
        gen_keys()
    if 'zoo' in which:
        gen_zoo()
    if 'zoo_frozen' in which:
        gen_zoo_frozen()
    if 'seeded' in which:
        gen_seeded()
    if 'pspnet' in which:
        gen_pspnet()
    if 'blocks' in which:
        gen_blocks()
    if 'eval' in which:
        gen_eval()
    if 'train' in which:
        gen_train()
    if 'frozen' in which:
        gen_frozen()
