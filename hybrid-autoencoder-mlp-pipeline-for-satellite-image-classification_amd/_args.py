"""Host-side argument checks and the workspace allocation shared by the modules over latents and class maps; no module's own."""
import numbers

import torch

from ._lib import check

MAX_L = 256


def _rows_arg(t, what, shape="[rows, L]", most=2 ** 31 - 1):
    """(rows, width) of a float32 [rows, L] latent, centroid, query or bank tensor, 1 <= L <= MAX_L and 1 <= rows <= most."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be a float32 tensor {shape}")
    n, width = int(t.shape[0]), int(t.shape[1])
    if not 1 <= width <= MAX_L:
        raise RuntimeError(f"the latent width of {what} must be in 1..{MAX_L}, got {width}")
    if not 1 <= n <= most:
        raise RuntimeError(f"the number of rows of {what} must be in 1..{'2^31-1' if most == 2 ** 31 - 1 else most}, got {n}")
    return n, width


def _int_arg(v, name, lo, hi):
    """An integer argument in lo..hi (bool is no integer here)."""
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= int(v) <= hi:
        raise RuntimeError(f"{name} must be an integer in {lo}..{hi}, got {v!r}")
    return int(v)


def _label_counts(labels, k):
    """Rows per label in [0, k), int64 [k] (integer adds: exact; -1 lands in the dropped slot 0)."""
    return torch.zeros(k + 1, dtype=torch.int64, device=labels.device).scatter_add_(0, labels + 1, torch.ones_like(labels))[1:]


def _alloc_workspace(nbytes, device, or_none=False):
    """The uint8 workspace of the `nbytes` an ``eae_*_workspace_bytes`` call returned (negative: its error, raised); or_none: None for 0."""
    check(min(int(nbytes), 0))
    return None if or_none and not nbytes else torch.empty(nbytes, dtype=torch.uint8, device=device)
