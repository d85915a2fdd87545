"""Nodata / mask helpers of eae_amd.scene that need no GPU: the invalid-pixel threshold, the valid-coverage count of the blend, and
the argument checks that run before any device work."""
import pytest
import torch

from eae_amd import scene as S


@pytest.mark.parametrize("patch,max_invalid,t", [(64, 0.0, 0), (64, 0.5, 2048), (64, 1.0 - 1e-12, 4095), (64, 1 / 4096, 1),
                                                 (64, 0.999 / 4096, 0), (128, 0.0, 0), (128, 0.25, 4096),
                                                 (128, 1.0 - 1e-12, 128 * 128 - 1)])
def test_invalid_threshold_edges(patch, max_invalid, t):
    assert S.invalid_threshold(patch, max_invalid) == t


@pytest.mark.parametrize("bad", [1.0, -0.01, float("nan"), float("inf"), 2, True, "0.1", None])
def test_invalid_threshold_rejects(bad):
    with pytest.raises(RuntimeError):
        S.invalid_threshold(64, bad)


def _brute_coverage(valid, k):
    n_h, n_w = valid.shape
    out = torch.zeros((n_h + k - 1, n_w + k - 1), dtype=torch.int64)
    for i in range(n_h):
        for j in range(n_w):
            if valid[i, j]:
                out[i:i + k, j:j + k] += 1
    return out


@pytest.mark.parametrize("n_h,n_w,k,seed", [(1, 1, 1, 0), (3, 5, 2, 1), (4, 2, 4, 2), (6, 7, 8, 3), (9, 4, 1, 4), (5, 11, 3, 5)])
def test_valid_coverage_matches_brute_force(n_h, n_w, k, seed):
    g = torch.Generator().manual_seed(seed)
    valid = torch.rand((n_h, n_w), generator=g) < 0.6
    got = S.valid_coverage(valid, k)
    assert got.dtype == torch.int64 and got.shape == (n_h + k - 1, n_w + k - 1)
    assert torch.equal(got, _brute_coverage(valid, k))
    # every window valid: the plain blend's coverage
    assert torch.equal(S.valid_coverage(torch.ones((n_h, n_w), dtype=torch.bool), k), S.cell_coverage(n_h, n_w, k))
    assert S.valid_coverage(torch.zeros((n_h, n_w), dtype=torch.bool), k).sum() == 0


def test_valid_coverage_rejects():
    for args in [(torch.ones((2, 3), dtype=torch.int64), 2), (torch.ones(3, dtype=torch.bool), 2),
                 (torch.ones((2, 3), dtype=torch.bool), 0), (torch.ones((0, 3), dtype=torch.bool), 1)]:
        with pytest.raises(RuntimeError):
            S.valid_coverage(*args)


@pytest.mark.parametrize("dtype,nodata", [(torch.uint8, 256), (torch.uint8, -1), (torch.uint8, 1.5), (torch.uint8, float("nan")),
                                          (torch.uint16, 65536), (torch.uint16, float("nan")), (torch.uint16, 0.25),
                                          (torch.float32, "0"), (torch.uint8, True)])
def test_nodata_rejected(dtype, nodata):
    with pytest.raises(RuntimeError):
        S._nodata_arg(dtype, nodata)


def test_nodata_accepted():
    assert S._nodata_arg(torch.uint8, None) == (S._NODATA_NONE, 0.0)
    assert S._nodata_arg(torch.uint8, 0) == (S._NODATA_VALUE, 0.0)
    assert S._nodata_arg(torch.uint8, 255.0) == (S._NODATA_VALUE, 255.0)          # rasterio reports nodata as a float
    assert S._nodata_arg(torch.uint16, 65535) == (S._NODATA_VALUE, 65535.0)
    assert S._nodata_arg(torch.float32, float("nan"))[0] == S._NODATA_NAN
    assert S._nodata_arg(torch.float32, -9999) == (S._NODATA_VALUE, -9999.0)


def test_host_arguments_rejected_before_device_work():
    """CPU tensors: every check below must fire before anything would touch a device."""
    scene = torch.zeros((3, 100, 100), dtype=torch.uint8)
    bad = [
        lambda: S._invalid_args(scene, 0, None, "most"),                                   # unknown rule
        lambda: S._invalid_args(scene, 300, None, "all"),                                  # outside uint8
        lambda: S._invalid_args(scene, None, torch.zeros((100, 99), dtype=torch.bool), "all"),   # mask shape
        lambda: S._invalid_args(scene, None, torch.zeros((100, 100), dtype=torch.int32), "all"),  # mask dtype
        lambda: S._invalid_args(scene.to(torch.int16), 0, None, "all"),                    # scene dtype
        lambda: S._windows_arg(torch.zeros(3, dtype=torch.int32), scene.device, 10, True),    # ids dtype
        lambda: S._windows_arg(torch.zeros((1, 3), dtype=torch.int64), scene.device, 10, True),  # 2-D
        lambda: S._windows_arg(torch.zeros(0, dtype=torch.int64), scene.device, 10, False),   # empty (encode)
        lambda: S._windows_arg(torch.tensor([0, 10]), scene.device, 10, True),             # outside the grid
        lambda: S._windows_arg(torch.tensor([-1, 3]), scene.device, 10, True),
    ]
    for fn in bad:
        with pytest.raises(RuntimeError):
            fn()
    m = S._mask_arg(scene, torch.ones((100, 100), dtype=torch.bool))
    assert m.dtype == torch.uint8 and int(m.sum()) == 100 * 100
    assert S._windows_arg(torch.zeros(0, dtype=torch.int64), scene.device, 10, True).numel() == 0
