"""Restatement of the two logit-distillation losses of csrc/distill.hip, dtype-generic (the tests run it in f32 and f64).

s, t: (B, C, h, w) student / teacher logits, T > 0 the temperature; every pixel counts; the teacher is a constant.
pixel  : p = softmax_c(t / T), q = softmax_c(s / T) per pixel,           loss = T^2 / (B h w) * sum p (log p - log q)
channel: p = softmax_i(t / T), q = softmax_i(s / T) over the h w positions of each (b, c) plane,
                                                                         loss = T^2 / (B C)   * sum p (log p - log q)
Both through log_softmax (over the class axis, or over the flattened position axis); the gradient comes from autograd.
"""
import torch
from torch.nn import functional as F

KINDS = ('pixel', 'channel')


def units(shape, kind):
    """(number of softmax units, terms per unit) of a (B, C, h, w) shape"""
    B, C, h, w = shape
    return (B * h * w, C) if kind == 'pixel' else (B * C, h * w)


def distillation_loss(student, teacher, temperature=1.0, kind='pixel'):
    if kind not in KINDS:
        raise ValueError(kind)
    s, t = student / temperature, teacher.detach() / temperature
    if kind == 'channel':
        s, t = s.flatten(2), t.flatten(2)
    axis = 1 if kind == 'pixel' else 2
    lq, lp = F.log_softmax(s, dim=axis), F.log_softmax(t, dim=axis)
    n, _ = units(student.shape, kind)
    return (lp.exp() * (lp - lq)).sum() * (temperature ** 2 / n)


def grad_closed_form(student, teacher, temperature, kind):
    """T / #units * (q - p)"""
    s, t = student / temperature, teacher / temperature
    shape = s.shape
    if kind == 'channel':
        s, t = s.flatten(2), t.flatten(2)
    axis = 1 if kind == 'pixel' else 2
    n, _ = units(shape, kind)
    return ((F.softmax(s, dim=axis) - F.softmax(t, dim=axis)) * (temperature / n)).reshape(shape)


def loss_and_grad(student, teacher, dtype, temperature, kind):
    """The restatement run in `dtype`; (loss, gradient with respect to the student by autograd)."""
    x = student.detach().to(dtype).clone().requires_grad_(True)
    loss = distillation_loss(x, teacher.detach().to(dtype), temperature, kind)
    loss.backward()
    return loss.detach(), x.grad.detach()
