"""Module shells with the reference notebook's signatures and state-dict layout.

``Encoder`` (R.md:287-313), ``Decoder`` (R.md:361-389), ``SupervisedAutoencoder`` (R.md:416-433) and
``MLP`` (R.md:2549-2566) keep the reference's constructor arguments, attribute names (``.encoder``,
``.decoder_input``, ``.decoder``, ``.enc``, ``.dec``, ``.classifier``, ``.net``), ``forward`` return
values and the 59-/16-tensor state-dict key layout, so checkpoints interchange both ways.

The layer objects inside the ``nn.Sequential`` containers are *parameter holders only*: they are
created with the same torch initialisers in the same order as the reference (so the same
``torch.manual_seed`` gives bit-identical initial weights) but their ``forward`` is disabled --
all arithmetic runs in the HIP engine (``engine.py`` -> ``csrc/`` through the C ABI of
``include/eae.h``).  There is no CPU or torch-eager fallback: calling ``forward`` without a HIP
device and the built extension raises.
"""
from __future__ import annotations

import torch
import torch.nn as nn


def _no_forward(self, *a, **k):
    raise RuntimeError(
        f"{type(self).__name__} is a parameter holder of the MI355X HIP engine; its arithmetic is not "
        "available as a stand-alone torch op. Call the owning Encoder/Decoder/SupervisedAutoencoder/MLP.")


class ConvS2Params(nn.Conv2d):
    """weight [Cout,Cin,3,3], bias [Cout] of a 3x3 stride-2 pad-1 convolution (R.md:292)."""
    forward = _no_forward


class DeconvS2Params(nn.ConvTranspose2d):
    """weight [Cin,Cout,3,3], bias [Cout] of a 3x3 stride-2 pad-1 output_padding-1 transposed conv (R.md:370)."""
    forward = _no_forward


class BatchNorm2dParams(nn.BatchNorm2d):
    forward = _no_forward


class BatchNorm1dParams(nn.BatchNorm1d):
    forward = _no_forward


class LinearParams(nn.Linear):
    forward = _no_forward


class _Marker(nn.Module):
    """Parameter-less placeholder keeping the reference's Sequential indices (ReLU, Flatten, ...)."""

    def __init__(self, what):
        super().__init__()
        self.what = what

    def extra_repr(self):
        return self.what

    forward = _no_forward


def _bands(n, what):
    """Image band count of the engine's edge layers: 1..16 (3 = RGB, the reference's value)."""
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= 16:
        raise ValueError(f"{what} must be an integer in 1..16 (image bands), got {n!r}")
    return int(n)


def _engine():
    from . import engine
    return engine


class Encoder(nn.Module):
    """R.md:287-313. forward(x [B,in_channels,H,W] fp32) -> z [B,latent_dim].  in_channels: image bands, 1..16 (the reference's
    RGB is 3); only conv1's weight [32,in_channels,3,3] depends on it."""

    def __init__(self, latent_dim, image_size=64, in_channels=3):
        super().__init__()
        self.latent_dim = int(latent_dim)
        self.image_size = int(image_size)
        self.in_channels = _bands(in_channels, "in_channels")
        fmap = self.image_size // 16
        self.encoder = nn.Sequential(
            ConvS2Params(self.in_channels, 32, 3, stride=2, padding=1), BatchNorm2dParams(32), _Marker("ReLU"),
            ConvS2Params(32, 64, 3, stride=2, padding=1), BatchNorm2dParams(64), _Marker("ReLU"),
            ConvS2Params(64, 128, 3, stride=2, padding=1), BatchNorm2dParams(128), _Marker("ReLU"),
            ConvS2Params(128, 256, 3, stride=2, padding=1), BatchNorm2dParams(256), _Marker("ReLU"),
            _Marker("Flatten"),
            LinearParams(256 * fmap * fmap, self.latent_dim),
        )

    def forward(self, x):
        return _engine().encoder_forward(self, x)


class Decoder(nn.Module):
    """R.md:361-389. forward(z [B,latent_dim]) -> x_hat [B,out_channels,H,W] in (0,1).  out_channels: image bands, 1..16 (3 = RGB);
    only deconv4's weight [32,out_channels,3,3] and bias [out_channels] depend on it."""

    def __init__(self, latent_dim, image_size=64, out_channels=3):
        super().__init__()
        self.latent_dim = int(latent_dim)
        self.image_size = int(image_size)
        self.out_channels = _bands(out_channels, "out_channels")
        fmap = self.image_size // 16
        self.decoder_input = LinearParams(self.latent_dim, 256 * fmap * fmap)
        self.decoder = nn.Sequential(
            _Marker("Unflatten(1,(256,h,w))"),
            DeconvS2Params(256, 128, 3, stride=2, padding=1, output_padding=1), BatchNorm2dParams(128), _Marker("ReLU"),
            DeconvS2Params(128, 64, 3, stride=2, padding=1, output_padding=1), BatchNorm2dParams(64), _Marker("ReLU"),
            DeconvS2Params(64, 32, 3, stride=2, padding=1, output_padding=1), BatchNorm2dParams(32), _Marker("ReLU"),
            DeconvS2Params(32, self.out_channels, 3, stride=2, padding=1, output_padding=1),
            _Marker("Sigmoid"),
        )

    def forward(self, z):
        return _engine().decoder_forward(self, z)


class SupervisedAutoencoder(nn.Module):
    """R.md:416-433. forward(x) -> (x_hat, logits, z); x and x_hat are [B,in_channels,H,W]."""

    def __init__(self, latent_dim, num_classes=10, image_size=64, in_channels=3):
        super().__init__()
        self.latent_dim = int(latent_dim)
        self.num_classes = int(num_classes)
        self.in_channels = _bands(in_channels, "in_channels")
        self.enc = Encoder(latent_dim, image_size, in_channels=self.in_channels)
        self.dec = Decoder(latent_dim, image_size, out_channels=self.in_channels)
        self.classifier = nn.Sequential(
            LinearParams(self.latent_dim, 128),
            _Marker("ReLU"),
            LinearParams(128, self.num_classes),
        )
        _engine().register_children(self, (self.enc, self.dec))

    def forward(self, x):
        return _engine().autoencoder_forward(self, x)


MLP_HIDDEN, MLP_DROPOUT = (128, 64), (0.3, 0.0)          # the reference's classifier (R.md:2549-2566)


def _mlp_arch(hidden, dropout):
    """(hidden, dropout) as tuples: 1..4 widths in 1..512, one rate in [0, 1) per hidden layer (a scalar: that rate everywhere)."""
    try:
        hidden = tuple(hidden)
    except TypeError:
        raise ValueError(f"hidden must be a sequence of 1..4 widths, got {hidden!r}") from None
    if not 1 <= len(hidden) <= 4:
        raise ValueError(f"hidden must hold 1..4 widths, got {len(hidden)}")
    for w in hidden:
        if isinstance(w, bool) or int(w) != w or not 1 <= int(w) <= 512:
            raise ValueError(f"every hidden width must be an integer in 1..512, got {w!r}")
    hidden = tuple(int(w) for w in hidden)
    if isinstance(dropout, (int, float)):
        dropout = (dropout,) * len(hidden)
    dropout = tuple(float(p) for p in dropout)
    if len(dropout) != len(hidden):
        raise ValueError(f"dropout must be a scalar or one rate per hidden layer ({len(hidden)}), got {len(dropout)}")
    for p in dropout:
        if not 0.0 <= p < 1.0:
            raise ValueError(f"every dropout rate must lie in [0, 1), got {p!r}")
    return hidden, dropout


class MLP(nn.Module):
    """R.md:2549-2566. forward(x [B,input_dim]) -> logits [B,num_classes].

    hidden: 1..4 hidden widths, each in 1..512; dropout: one rate in [0, 1) per hidden layer, or a scalar for all of them.  ``net`` is
    the Sequential the reference would write for them: Linear, BatchNorm1d, ReLU and -- only where the rate is above 0 -- Dropout per
    hidden layer, then the last Linear; the defaults are the reference's classifier with its net.0 ... net.7 state dict."""

    def __init__(self, input_dim, num_classes=10, hidden=MLP_HIDDEN, dropout=MLP_DROPOUT):
        super().__init__()
        self.input_dim = int(input_dim)
        self.num_classes = int(num_classes)
        self.hidden, self.dropout = _mlp_arch(hidden, dropout)
        layers, k = [], self.input_dim
        for w, p in zip(self.hidden, self.dropout):
            layers += [LinearParams(k, w), BatchNorm1dParams(w), _Marker("ReLU")]
            if p > 0:
                layers.append(_Marker(f"Dropout({p})"))
            k = w
        layers.append(LinearParams(k, self.num_classes))
        self.net = nn.Sequential(*layers)

    def forward(self, x):
        from . import mlp_engine
        return mlp_engine.mlp_forward(self, x)


def mlp_from_state_dict(sd, dropout=None):
    """The classifier of a checkpoint (``MLP.state_dict()``, e.g. a saved MLP_GLOBAL_BEST.pt), with the state loaded: input_dim, hidden
    and num_classes come from the Linear weight shapes, the places of the Dropout markers from the gaps in the ``net.<i>`` indices.  A
    rate is not part of a checkpoint: 0.3 where a marker is, unless ``dropout`` (a rate per hidden layer) gives them -- it must agree
    with the checkpoint about where a marker is."""
    idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith("net.") and k.endswith(".weight") and sd[k].dim() == 2})
    if not idx or idx[0] != 0:
        raise ValueError("not an MLP state dict: no net.0.weight of a Linear")
    hidden = tuple(int(sd[f"net.{i}.weight"].shape[0]) for i in idx[:-1])
    # a hidden layer takes 3 indices (Linear, BatchNorm1d, ReLU), 4 with a Dropout marker
    gaps = [b - a for a, b in zip(idx[:-1], idx[1:])]
    if not hidden or any(g not in (3, 4) for g in gaps):
        raise ValueError(f"not an MLP state dict: Linear layers at net indices {idx}")
    marked = [g == 4 for g in gaps]
    if dropout is None:
        rates = tuple(0.3 if m else 0.0 for m in marked)
    else:
        _, rates = _mlp_arch(hidden, dropout)
        if [p > 0 for p in rates] != marked:
            raise ValueError(f"dropout={dropout!r} disagrees with the checkpoint, whose Dropout markers follow hidden layers "
                             f"{[l for l, m in enumerate(marked) if m]}")
    clf = MLP(int(sd["net.0.weight"].shape[1]), int(sd[f"net.{idx[-1]}.weight"].shape[0]), hidden=hidden, dropout=rates)
    clf.load_state_dict(sd)
    return clf
