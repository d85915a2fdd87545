"""Per-epoch learning-rate schedules for the fit functions (train.fit_autoencoder, fit_autoencoder_group, fit_mlp and the grid drivers:
``lr_schedule=``).  The reference holds the learning rate fixed for a whole run and names "learning-rate scheduling or gradient clipping"
first in its future work; every step entry of the engines takes the learning rate per call (graph replay refreshes it per step too), so
a schedule is host code only.

Protocol -- any object with

    lr(epoch, base_lr) -> float     called before each epoch's train phase (epoch counts from 0; base_lr = the configuration's lr)
    observe(val_loss)               called after each validation phase

The fit functions take a zero-argument FACTORY (``lr_schedule=lambda: plateau(patience=3)``) and build a fresh instance per
configuration, so every member of a group keeps its own state and its own learning rate.
"""
from __future__ import annotations

import math


class cosine:
    """Linear warm-up over `warmup` epochs (base_lr * (epoch + 1) / warmup), then cosine annealing to `floor` over the remaining
    T = num_epochs - warmup epochs: floor + (base_lr - floor) * (1 + cos(pi * t / T)) / 2 with t = epoch - warmup.  With warmup=0
    this is torch's CosineAnnealingLR(T_max=num_epochs, eta_min=floor) in closed form; epochs past num_epochs stay at `floor`."""

    def __init__(self, num_epochs, warmup=0, floor=0.0):
        self.num_epochs, self.warmup, self.floor = int(num_epochs), int(warmup), float(floor)
        if self.warmup < 0 or self.num_epochs <= self.warmup:
            raise ValueError("cosine: need 0 <= warmup < num_epochs")

    def lr(self, epoch, base_lr):
        base_lr = float(base_lr)
        if epoch < self.warmup:
            return base_lr * (epoch + 1) / self.warmup
        T = self.num_epochs - self.warmup
        t = min(epoch - self.warmup, T)
        return self.floor + (base_lr - self.floor) * (1.0 + math.cos(math.pi * t / T)) / 2.0

    def observe(self, val_loss):
        pass


class plateau:
    """torch's ReduceLROnPlateau(mode="min", threshold_mode="rel", cooldown=0, eps=1e-8) on the validation loss: a loss below
    best * (1 - threshold) is an improvement; after more than `patience` epochs without one the learning rate is multiplied by
    `factor` (not below `min_lr`; a change of at most 1e-8 is not applied) and the count starts again."""

    def __init__(self, factor=0.5, patience=5, threshold=1e-4, min_lr=0.0):
        if not factor < 1.0:
            raise ValueError("plateau: factor must be < 1")
        self.factor, self.patience, self.threshold, self.min_lr = float(factor), int(patience), float(threshold), float(min_lr)
        self.best, self.num_bad, self._lr = math.inf, 0, None

    def lr(self, epoch, base_lr):
        if self._lr is None:
            self._lr = float(base_lr)
        return self._lr

    def observe(self, val_loss):
        val_loss = float(val_loss)
        if val_loss < self.best * (1.0 - self.threshold):
            self.best, self.num_bad = val_loss, 0
        else:
            self.num_bad += 1
        if self.num_bad > self.patience:
            if self._lr is not None:
                new = max(self._lr * self.factor, self.min_lr)
                if self._lr - new > 1e-8:
                    self._lr = new
            self.num_bad = 0
