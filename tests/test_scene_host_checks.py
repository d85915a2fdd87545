"""One host-side check for every model-running scene function (`scene._host_plan`; no GPU needed): the same bad argument is
reported by its own message whichever function is given it, before the library is loaded or a device is asked for, and with valid
arguments a host scene fails on the one thing missing, the device."""
import inspect

import pytest
import torch

import eae_amd
from eae_amd import _lib

NAMES = ("encode_scene", "classify_scene", "scene_reconstruction_error", "reconstruct_scene", "evaluate_scene", "cluster_scene",
         "similar_windows", "knn_classify_scene")
# an empty ``windows`` is a legal window set where the maps simply stay unwritten (label -1, NaN); where latents are returned or
# searched there is nothing to return
EMPTY_IS_VALID = ("classify_scene", "scene_reconstruction_error", "reconstruct_scene", "evaluate_scene")

BAD = {
    "nodata=0.5": dict(nodata=0.5),
    "mask 5x5": dict(mask=torch.zeros((5, 5), dtype=torch.bool)),
    "float windows": dict(windows=torch.tensor([0.5, 1.0])),
    "empty windows": dict(windows=torch.zeros(0, dtype=torch.int64)),
    "windows + nodata": dict(windows=torch.tensor([0, 1]), nodata=0),
    "stride=65": dict(stride=65),
    "border=wrap": dict(border="wrap"),
    "rule=some": dict(rule="some"),
    "max_invalid=1.0": dict(max_invalid=1.0),
    "two-value divisor": dict(divisor=[255.0, 255.0]),
    "batch=0": dict(batch=0),
    "4-band scene": dict(scene=torch.zeros((4, 160, 224), dtype=torch.uint8)),
}


@pytest.fixture(scope="module")
def calls():
    """name -> (function, valid keyword arguments) on a host scene uint8 [3,160,224]: a 2 x 3 grid at patch 64."""
    torch.manual_seed(0)
    ae = eae_amd.SupervisedAutoencoder(64, 10, image_size=64, in_channels=3)
    mlp = eae_amd.MLP(64, 10)
    scene = torch.zeros((3, 160, 224), dtype=torch.uint8)
    own = {
        "encode_scene": dict(encoder=ae),
        "classify_scene": dict(encoder=ae, mlp=mlp),
        "scene_reconstruction_error": dict(autoencoder=ae),
        "reconstruct_scene": dict(autoencoder=ae),
        "evaluate_scene": dict(encoder=ae, mlp=mlp, truth=torch.zeros((160, 224), dtype=torch.uint8)),
        "cluster_scene": dict(encoder=ae, k=2),
        "similar_windows": dict(encoder=ae, query=torch.tensor([0, 5]), k=2),
        "knn_classify_scene": dict(encoder=ae, bank=torch.zeros((9, 64)), bank_labels=torch.zeros(9, dtype=torch.int64), k=3, num_classes=4),
    }
    return {name: (getattr(eae_amd, name), dict(scene=scene, **kw)) for name, kw in own.items()}


def _message(fn, kwargs):
    with pytest.raises(RuntimeError) as e:
        fn(**kwargs)
    return str(e.value)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", list(BAD))
def test_bad_argument_is_rejected_before_the_device(calls, name, case, monkeypatch):
    fn, ok = calls[name]
    bad = BAD[case]
    if not set(bad) <= set(inspect.signature(fn).parameters):
        return                                                   # the function does not take this argument
    msg = _message(fn, {**ok, **bad})
    if case == "empty windows" and name in EMPTY_IS_VALID:
        assert "HIP device" in msg
        return
    assert "HIP device" not in msg, msg

    def no_library():
        raise RuntimeError("the library must not be loaded before the host checks have passed")
    monkeypatch.setattr(_lib, "load", no_library)
    assert _message(fn, {**ok, **bad}) == msg


def test_every_function_takes_the_shared_arguments(calls):
    """Nothing in the table is skipped by accident: what a function lacks is what its signature really does not have."""
    lacks = {name: sorted(c for c in BAD if not set(BAD[c]) <= set(inspect.signature(calls[name][0]).parameters)) for name in NAMES}
    assert lacks.pop("encode_scene") == ["mask 5x5", "max_invalid=1.0", "nodata=0.5", "rule=some", "windows + nodata"]
    assert all(v == [] for v in lacks.values()), lacks


@pytest.mark.parametrize("name", NAMES)
def test_valid_arguments_need_only_the_device(calls, name):
    fn, ok = calls[name]
    assert "HIP device" in _message(fn, ok)
    assert "HIP device" in _message(fn, {**ok, "border": "reflect", "anchor": "origin", "windows": torch.tensor([3, 0, 11])})   # 3 x 4 grid
