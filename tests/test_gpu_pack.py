"""Every weight pack of the engine, bit for bit, against the NumPy layouts of tests/pack_ref.py.

pack_all_kernel (csrc/eae_misc.hip) turns the fp32 parameter arena into the layouts the MFMA kernels read; which of its code paths
fills a pack depends on the pack's shape, and the engine only ever launches its flattened form (ensure_packed).  A pack is a
permutation plus one rounding, so every comparison here is equality of raw bytes: no tolerance anywhere in this file.

Each case: a fresh context with max_batch 1, fp32 weights drawn from a seeded normal distribution (NOT bf16-rounded: the kernel's
rounding is under test), then eae_debug_fill_packs(0xFF) -- every bf16, fp32 and e4m3 element of the arena reads as NaN until a
workgroup has written it, the zero padding included --, eae_params_changed, a batch-1 eval forward, and a read of every pack."""
import ctypes as C

import numpy as np
import pytest
import torch

import pack_ref as R

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -2, -4
DEBUG_PACK = 6


@pytest.fixture(scope="module")
def lib():
    from eae_amd import _lib
    return _lib.load()


def random_state(h, w, latent, bands, seed, classes=10):
    """state_dict of fp32 normal draws (std 0.05: weights of the usual size, many of them e4m3 subnormals at scale 1)."""
    rng = np.random.default_rng(seed)
    return {n: (rng.standard_normal(s, dtype=np.float32) * np.float32(0.05)) for n, s in R.param_shapes(h, w, latent, classes, bands).items()}


class Ctx:
    """One engine context on the C ABI (the Python engine is square-only; the pack shapes here are not)."""

    def __init__(self, lib, h, w, latent, bands, max_batch=1, quant=0, train=False, classes=10):
        from eae_amd import _lib
        self.lib, self.check, self._lib = lib, _lib.check, _lib
        self.h, self.w, self.latent, self.bands, self.classes = h, w, latent, bands, classes
        self.cfg = _lib.EaeConfig(latent, classes, h, w, max_batch, quant, 0, bands)
        poff, boff = (C.c_longlong * 39)(), (C.c_longlong * 15)()
        self.check(lib.eae_ae_layout(C.byref(self.cfg), poff, boff))
        self.poff = list(poff)
        dev = torch.device("cuda:0")
        n = self.poff[38]
        self.params = torch.zeros(n, dtype=torch.float32, device=dev)
        # gradient and moment arenas only where a case steps the optimizer (16.7 M-element projections at 256 px)
        self.grads, self.m, self.v = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(3)) if train else (None, None, None)
        self.bn = torch.zeros(boff[14], dtype=torch.float32, device=dev)
        for l in range(7):
            self.bn[boff[2 * l + 1]: boff[2 * l + 2]] = 1.0                     # running_var
        self.nbt = torch.zeros(7, dtype=torch.int64, device=dev)
        self.loss_last = torch.zeros(4, dtype=torch.float32, device=dev)
        self.ctx = C.c_void_p()
        self.check(lib.eae_create(C.byref(self.cfg), C.byref(self.ctx)))
        ptr = self._ptr
        self.check(lib.eae_bind(self.ctx, ptr(self.params), ptr(self.grads), ptr(self.m), ptr(self.v), ptr(self.bn), ptr(self.nbt)))
        rng = np.random.default_rng(99)
        self.x = torch.from_numpy(rng.random((max_batch, bands, h, w), dtype=np.float32)).to(dev)
        self.labels = torch.from_numpy(rng.integers(0, classes, max_batch).astype(np.int64)).to(dev)
        self.x_hat = torch.empty_like(self.x)

    @staticmethod
    def _ptr(t):
        return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())

    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def close(self):
        if self.ctx:
            torch.cuda.synchronize()
            self.lib.eae_destroy(self.ctx)
            self.ctx = None

    def upload(self, sd):
        host = np.zeros(self.poff[38], np.float32)
        for i, n in enumerate(R.PARAM_NAMES):
            host[self.poff[i]: self.poff[i] + sd[n].size] = sd[n].ravel()
        self.params.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()

    def download(self):
        host = self.params.cpu().numpy()
        shapes = R.param_shapes(self.h, self.w, self.latent, self.classes, self.bands)
        return {n: host[self.poff[i]: self.poff[i] + int(np.prod(shapes[n]))].reshape(shapes[n]).copy() for i, n in enumerate(R.PARAM_NAMES)}

    def io(self, B, train):
        ptr = self._ptr
        return self._lib.EaeStepIO(ptr(self.x), ptr(self.labels), B, int(train), 1, 35.0, ptr(self.x_hat), None, None, None, ptr(self.loss_last))

    def fill_and_pack(self):
        """0xFF over the pack arena, parameters declared changed, one batch-1 eval forward."""
        self.check(self.lib.eae_debug_fill_packs(self.ctx, 0xFF))
        self.check(self.lib.eae_params_changed(self.ctx))
        self.eval_forward()

    def eval_forward(self):
        io = self.io(1, False)
        self.check(self.lib.eae_ae_forward(self.ctx, self._stream(), C.byref(io)))
        torch.cuda.synchronize()

    def pack_len(self, idx):
        return int(self.lib.eae_debug_read(self.ctx, DEBUG_PACK, idx, None, 0))

    def read_pack(self, idx, dtype):
        n = self.pack_len(idx)
        assert n > 0, (idx, n, self.lib.eae_last_error())
        buf = np.empty(n, np.uint8)
        got = int(self.lib.eae_debug_read(self.ctx, DEBUG_PACK, idx, buf.ctypes.data_as(C.c_void_p), n))
        assert got == n, (idx, got, n)
        return buf.view(dtype)


def assert_packs_equal(ctx, ref, only=None):
    """Every pack of `ref` (pack index -> bits) equals the arena's, byte for byte."""
    bad = []
    for idx in sorted(ref):
        if only is not None and idx not in only:
            continue
        want = ref[idx]
        n = ctx.pack_len(idx)
        if n != want.nbytes:
            bad.append(f"{R.PACK_LABEL[idx]}: length {n} bytes, expected {want.nbytes}")
            continue
        got = ctx.read_pack(idx, want.dtype).reshape(want.shape)
        if not np.array_equal(got, want):
            ne = got != want
            unwritten = int((ne & (got == np.iinfo(want.dtype).max)).sum())        # still the 0xFF fill
            first = [tuple(int(v) for v in i) for i in np.argwhere(ne)[:4]]
            bad.append(f"{R.PACK_LABEL[idx]} {want.shape}: {int(ne.sum())} of {want.size} elements differ, {unwritten} of them never "
                       f"written (NaN fill); first at {first}")
    assert not bad, "\n".join(bad)


# image h x w, latent width, bands: the path each case exists for
CASES = [
    pytest.param(64, 64, 64, 3, id="64x64-L64-3b"),        # mid KPERM path at P = 16, ROWPERM 8-wide, ROWPERM_TRANS fallback, CP = 4
    pytest.param(64, 64, 50, 1, id="64x64-L50-1b"),        # latent padding (w1p, bep), ROWPERM fallback (lv % 8 != 0), CP = 8
    pytest.param(64, 64, 48, 13, id="64x64-L48-13b"),      # lv < Lp with lv % 8 == 0, CP = 16
    pytest.param(128, 128, 256, 3, id="128x128-L256-3b"),  # both LDS-tile paths at exactly 1024 tiles
    pytest.param(128, 128, 192, 3, id="128x128-L192-3b"),  # just below the threshold: mid path at P = 64
    pytest.param(128, 256, 128, 3, id="128x256-L128-3b"),  # P = 128: 1024 tiles with two 64-position chunks
    pytest.param(256, 256, 256, 3, id="256x256-L256-3b"),  # 4096 tiles on at most 1024 workgroups: the tile loops stride
    pytest.param(256, 256, 200, 3, id="256x256-L200-3b"),  # float4 branch with a partial last latent tile, zero rows 200..255
    pytest.param(256, 256, 201, 3, id="256x256-L201-3b"),  # scalar (!vec) branch, ROWPERM fallback at a big shape
]


@pytest.mark.parametrize("h,w,latent,bands", CASES)
def test_engine_packs_equal_numpy_layouts(lib, h, w, latent, bands):
    sd = random_state(h, w, latent, bands, seed=1000 + h + 3 * w + 7 * latent + bands)
    ref = R.packs(sd)
    ctx = Ctx(lib, h, w, latent, bands)
    try:
        ctx.upload(sd)
        ctx.fill_and_pack()
        assert_packs_equal(ctx, ref)
        # the packs a context does not have
        if latent % 64 == 0:
            assert ctx.pack_len(R.W1P) == ERR_STATE and ctx.pack_len(R.BEP) == ERR_STATE
        assert ctx.pack_len(R.FP8_P1) == ERR_STATE and ctx.pack_len(R.FP8_P2 + 5) == ERR_STATE
        assert ctx.pack_len(34) == ERR_ARG and ctx.pack_len(-1) == ERR_ARG
    finally:
        ctx.close()


def test_read_contract_and_fill(lib):
    """bytes = 0 or a small buffer: the pack's full length comes back and no more than `bytes` are copied; the read packs nothing;
    the fill reaches every byte of every pack."""
    sd = random_state(64, 64, 50, 3, seed=7)
    ctx = Ctx(lib, 64, 64, 50, 3)
    try:
        ctx.upload(sd)
        lib.eae_debug_fill_packs(ctx.ctx, 0xFF)
        ref = R.packs(sd)
        for idx, want in ref.items():
            assert ctx.pack_len(idx) == want.nbytes, R.PACK_LABEL[idx]
            assert (ctx.read_pack(idx, np.uint8) == 0xFF).all(), R.PACK_LABEL[idx]          # filled, and reading did not pack
        buf = np.full(64, 0x5A, np.uint8)
        ctx.fill_and_pack()
        n = int(lib.eae_debug_read(ctx.ctx, DEBUG_PACK, R.WE1, buf.ctypes.data_as(C.c_void_p), 16))
        assert n == ref[R.WE1].nbytes
        assert np.array_equal(buf[:16], ref[R.WE1].view(np.uint8).ravel()[:16]) and (buf[16:] == 0x5A).all()
    finally:
        ctx.close()


def test_repack_after_optimizer_step(lib):
    """One train step (B = 2) moves every parameter: the next forward must pack the UPDATED arena, with and without the 0xFF fill."""
    sd = random_state(64, 64, 64, 3, seed=11)
    ctx = Ctx(lib, 64, 64, 64, 3, max_batch=2, train=True)
    try:
        ctx.upload(sd)
        ctx.fill_and_pack()
        assert_packs_equal(ctx, R.packs(sd))
        io = ctx.io(2, True)
        ctx.check(lib.eae_ae_train_step(ctx.ctx, ctx._stream(), C.byref(io), 1e-2))
        torch.cuda.synchronize()
        new = ctx.download()
        for n in ("enc.encoder.3.weight", "enc.encoder.13.weight", "dec.decoder_input.weight", "dec.decoder.10.weight"):
            assert np.isfinite(new[n]).all() and (new[n] != sd[n]).mean() > 0.25, n        # the step was applied (exact-zero gradients behind a ReLU stay put)
        ref = R.packs(new)
        assert not np.array_equal(ref[R.WE1], R.packs(sd)[R.WE1])
        ctx.eval_forward()                       # the optimizer step alone must have marked the packs stale
        assert_packs_equal(ctx, ref)
        ctx.check(lib.eae_debug_fill_packs(ctx.ctx, 0xFF))
        ctx.eval_forward()                       # ... and a full repack leaves nothing of the old packs or of the fill
        assert_packs_equal(ctx, ref)
    finally:
        ctx.close()


def test_grouped_forward_packs_each_member(lib):
    """eae_group_forward on three members of one shape with different weights: pack_all_kernel_g must take each member's own
    argument block (latent 48: padding packs, the 8-wide ROWPERM path, the mid KPERM path, the 3x3 path)."""
    sds = [random_state(64, 64, 48, 3, seed=20 + k) for k in range(3)]
    ctxs = [Ctx(lib, 64, 64, 48, 3) for _ in range(3)]
    try:
        from eae_amd import _lib
        for c, sd in zip(ctxs, sds):
            c.upload(sd)
            c.check(lib.eae_debug_fill_packs(c.ctx, 0xFF))
            c.check(lib.eae_params_changed(c.ctx))
        ios = (_lib.EaeStepIO * 3)(*[c.io(1, False) for c in ctxs])
        handles = (C.c_void_p * 3)(*[c.ctx for c in ctxs])
        _lib.check(lib.eae_group_forward(handles, 3, 0, Ctx._stream(), ios))
        torch.cuda.synchronize()
        for c, sd in zip(ctxs, sds):
            assert_packs_equal(c, R.packs(sd))
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------------------------------------------------------
# fp8 packs (quant = 1; smallest allowed shape 128 x 256, 3 bands)
# ---------------------------------------------------------------------------------------------------------------
FP8_SEED = 39       # chosen on the CPU so that the precondition below holds with margin (every layer >= 0.06 in log2)
# layer 0: both signs saturate; layer 3: negative only, so that its max |w| is attained by a negative weight (a maximum taken
# without the absolute value would report ~0.2 there and lead to another scale)
FP8_SPIKES = {0: [(5, 3, 1, 2, 1000.0), (60, 31, 0, 0, -1000.0)], 3: [(0, 0, 2, 2, -1000.0), (255, 127, 1, 1, -1000.0), (17, 5, 0, 1, -1000.0)]}


def _fp8_state():
    sd = random_state(128, 256, 64, 3, seed=FP8_SEED)
    for layer, spikes in FP8_SPIKES.items():                # far beyond 448 / s_w: the conversion must saturate to +-448
        for a, b, ky, kx, v in spikes:
            sd[R.W3_NAMES[layer]][a, b, ky, kx] = np.float32(v)
    return sd


def test_fp8_packs_saturation_and_scales(lib):
    sd = _fp8_state()
    amax = [float(np.abs(sd[n]).max()) for n in R.W3_NAMES]
    # precondition on the inputs, before the GPU is touched: 448 / (2 max|w|) is not within 1 % of a power of two, so the rounding of
    # the kernel's log2f cannot decide floor()
    for a in amax:
        lg = np.log2(448.0 / (2.0 * a))
        assert abs(lg - np.round(lg)) > np.log2(1.01), (FP8_SEED, amax)
    want_scales = [R.fp8_scale(a) for a in amax]
    assert want_scales[0] == 2.0 ** -3 and want_scales[3] == 2.0 ** -3 and min(want_scales[i] for i in (1, 2, 4, 5)) >= 256.0
    ref1 = R.packs(sd, quant_scales=[1.0] * 6)
    # the spikes saturate, and ordinary weights reach the subnormals
    assert (ref1[R.FP8_P1] == 0x7E).sum() == 1 and (ref1[R.FP8_P1] == 0xFE).sum() == 1 and (ref1[R.FP8_P2 + 3] == 0xFE).sum() == 3
    assert max(float(sd[R.W3_NAMES[3]].max()), 0.0) < 0.5
    assert ((ref1[R.FP8_P1 + 1] & 0x78) == 0).mean() > 0.1
    ctx = Ctx(lib, 128, 256, 64, 3, quant=1, train=True)
    try:
        out = (C.c_float * 18)()
        ctx.check(lib.eae_fp8_scales(ctx.ctx, out))
        assert list(out)[12:18] == [1.0] * 6                  # a fresh context: s_w = 1
        ctx.upload(sd)
        ctx.fill_and_pack()
        assert_packs_equal(ctx, ref1)
        # one calibration iteration (weights untouched) turns the reported max |w| into the scales of the next pack
        io = ctx.io(1, True)
        ctx.check(lib.eae_fp8_calibrate(ctx.ctx, ctx._stream(), C.byref(io), 1))
        torch.cuda.synchronize()
        got_sd = ctx.download()
        assert all(np.array_equal(got_sd[n], sd[n]) for n in R.PARAM_NAMES)
        ctx.check(lib.eae_fp8_scales(ctx.ctx, out))
        assert list(out)[12:18] == want_scales, (list(out)[12:18], want_scales)
        ctx.fill_and_pack()
        assert_packs_equal(ctx, R.packs(sd, quant_scales=want_scales))
    finally:
        ctx.close()
