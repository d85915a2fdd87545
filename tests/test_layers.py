"""The layer tables of csrc/eae_layers.h: the stand-alone host program layers_check.cpp compares everything derived from them with
the literal arrays they replaced, and the data-parallel cut points of dp.py name the same tensors as the module (no GPU)."""
import os
import shutil
import subprocess

import pytest

import eae_amd
from eae_amd import dp

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(eae_amd.__file__), "csrc")


def test_tables_equal_the_literals_they_replaced(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++ or clang++) on PATH")
    exe = str(tmp_path / "layers_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "layers_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("90 configurations, 0 differences"), r.stdout


def test_dp_constants_name_the_modules_tensors():
    params = dict(eae_amd.SupervisedAutoencoder(64).named_parameters())
    names = list(params)
    assert len(names) == dp.T_COUNT == 38
    assert (dp.CUT_CONVS_FC, dp.CUT_ENC_DEC, dp.CUT_FC_DECONVS) == (16, 18, 20)
    # encoder convolutions | latent projections: the encoder's Linear [latent][256 * 4 * 4]
    assert names[dp.CUT_CONVS_FC] == "enc.encoder.13.weight" and tuple(params[names[16]].shape) == (64, 4096)
    # encoder half | decoder half: the decoder's Linear [256 * 4 * 4][latent]
    assert names[dp.CUT_ENC_DEC] == "dec.decoder_input.weight" and tuple(params[names[18]].shape) == (4096, 64)
    # latent projections | transposed convolutions: deconv1 [256][128][3][3]
    assert names[dp.CUT_FC_DECONVS] == "dec.decoder.1.weight" and tuple(params[names[20]].shape) == (256, 128, 3, 3)
    assert names[dp.T_CONV3_W] == "enc.encoder.6.weight" and tuple(params[names[8]].shape) == (128, 64, 3, 3)
    # the C enum carries the same values under the same names
    src = open(os.path.join(CSRC, "eae_layers.h")).read()
    for name, tensor in (("CUT_CONVS_FC", "T_ENCFC_W"), ("CUT_ENC_DEC", "T_DECFC_W"), ("CUT_FC_DECONVS", "T_DECONV1_W")):
        assert f"{name} = {tensor}," in src or f"{name} = {tensor} " in src, name
    enum = src[src.index("enum EaeTensor {"):src.index("T_COUNT")]
    order = [t.strip() for t in enum.split("{", 1)[1].replace("\n", " ").split(",") if t.strip()]
    assert len(order) == 38
    assert (order[16], order[18], order[20], order[8]) == ("T_ENCFC_W", "T_DECFC_W", "T_DECONV1_W", "T_CONV3_W")
