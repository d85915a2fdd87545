"""Helpers shared by the GPU scene tests (test_gpu_scene.py, test_gpu_scene_nodata.py, test_gpu_scene_recon.py): seeded scenes, their
divisors, models with non-trivial running statistics, and the C scene descriptor."""
import ctypes as C

import torch

import eae_amd
from eae_amd import _lib

_MAX = {torch.uint8: 256, torch.uint16: 65536}


def _scene(c, h, w, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        s = torch.rand((c, h, w), generator=g) * 3.0
    else:
        s = torch.randint(0, _MAX[dtype], (c, h, w), generator=g, dtype=torch.int64).to(dtype)
    return s.cuda()


def _divisor(c, dtype):
    base = {torch.uint8: 255.0, torch.uint16: 10000.0, torch.float32: 1.5}[dtype]
    return [base * (1.0 + 0.1 * i) for i in range(c)]


def _model(c, seed=0, latent=64, batch=512, image_size=64, all_halves=False):
    """An eval-mode SupervisedAutoencoder with non-trivial running statistics (eval mode must use them) in the encoder, or with
    all_halves=True in every BatchNorm of the model, drawn in module order."""
    torch.manual_seed(seed)
    m = eae_amd.SupervisedAutoencoder(latent, 10, image_size=image_size, in_channels=c)
    m._eae_max_batch = batch                   # the engine's max_batch: the fused path's batch, and the staged path's
    with torch.no_grad():
        for mod in (m if all_halves else m.enc).modules():
            if hasattr(mod, "running_mean") and mod.running_mean is not None:
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 2.0)
    return m.cuda().eval()


def _mlp(latent=64, classes=10, seed=3):
    torch.manual_seed(seed)
    m = eae_amd.MLP(latent, classes)
    with torch.no_grad():
        for bn in (m.net[1], m.net[5]):
            bn.running_mean.uniform_(-0.3, 0.3)
            bn.running_var.uniform_(0.5, 2.0)
    return m.cuda().eval()


def _desc(scene, div, patch=64, stride=64, dtype=None):
    return _lib.EaeScene(C.c_void_p(scene.data_ptr()), C.c_void_p(0 if div is None else div.data_ptr()),
                         {torch.uint8: 0, torch.uint16: 1, torch.float32: 2}[scene.dtype] if dtype is None else dtype,
                         scene.shape[0], scene.shape[1], scene.shape[2], patch, stride)
