#!/usr/bin/env python3
"""Diagnostic: SHA-256 digests of what a few steps of one configuration leave behind -- parameter arena, gradient arena, BatchNorm
buffers with num_batches_tracked, loss scalars -- to compare two builds of the engine bit for bit (a refactor of the host code must
leave every digest as it is; digests of different compilers or devices are not comparable, so none are kept in the repository).

    tools/step_digest.py --list          the cases
    tools/step_digest.py CASE            one case in this process: prints `CASE params grads bn loss`
    tools/step_digest.py --all [CASE..]  every case (or the named ones), each in a fresh process with the environment switches it
                                         names; stops at the first case that fails
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = 5
ALPHA, LR = 35.0, 5e-3


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def _digest(engines):
    import torch
    torch.cuda.synchronize()
    return " ".join((_sha(*[e.params for e in engines]), _sha(*[e.grads for e in engines]),
                     _sha(*[t for e in engines for t in (e.bn_running, e.bn_nbt)]),
                     _sha(*[t for e in engines for t in (e.loss_accum, e.loss_last)])))


def _batch(B, bands=3, size=64, classes=10, seed=1234):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.rand((B, bands, size, size), generator=g).cuda(), torch.randint(0, classes, (B,), generator=g).cuda()


def _model(latent=64, size=64, bands=3, seed=0):
    import torch
    import eae_amd
    torch.manual_seed(seed)
    m = eae_amd.SupervisedAutoencoder(latent, 10, image_size=size, in_channels=bands).cuda()
    m.train()
    return m


def train(B=8, latent=64, size=64, bands=3, head=True, setup=None, graph=None):
    from eae_amd.engine import engine_for
    m = _model(latent, size, bands)
    eng = engine_for(m, max_batch=B)
    if graph is not None:
        eng.set_graph(graph)
    if setup:
        setup(eng)
    x, y = _batch(B, bands, size)
    if setup and eng.ignore_index is not None:
        y[::3] = eng.ignore_index
    for _ in range(STEPS):
        eng.train_step(x, y, ALPHA, LR, head=head)
    return _digest([eng])


def split_step():
    from eae_amd.engine import engine_for
    eng = engine_for(_model(), max_batch=8)
    x, y = _batch(8)
    for _ in range(STEPS):
        eng.grad_step_begin(x, y, ALPHA)
        eng.grad_step_end()
        eng.adam_step(LR)
    return _digest([eng])


def group3():
    from eae_amd.engine import AEEngine, engine_for
    models = [_model(seed=k) for k in range(3)]
    engines = [engine_for(m, max_batch=8) for m in models]
    batches = [_batch(8, seed=100 + k) for k in range(3)]
    for _ in range(STEPS):
        AEEngine.group_train_step(engines, [b[0] for b in batches], [b[1] for b in batches], [ALPHA, 10.0, 1.0], [LR, 1e-3, 2e-3])
    return _digest(engines)


def autograd(train_mode):
    import torch
    from eae_amd.engine import engine_for
    m = _model()
    m.train(train_mode)
    m._eae_max_batch = 8           # the workspace size of the engine that m(x) builds and every later engine_for(m) returns
    eng = engine_for(m)
    x, y = _batch(8)
    for _ in range(STEPS):
        x_hat, logits, z = m(x)
        loss = ALPHA * torch.nn.functional.mse_loss(x_hat, x) + torch.nn.functional.cross_entropy(logits, y) + 1e-3 * z.square().sum()
        loss.backward()
        eng.adam_step(LR)
    return _digest([eng])


def halves():
    import torch
    import eae_amd
    from eae_amd.engine import engine_for
    torch.manual_seed(0)
    enc, dec = eae_amd.Encoder(64).cuda(), eae_amd.Decoder(64).cuda()
    enc._eae_max_batch = dec._eae_max_batch = 8
    x, _ = _batch(8)
    for mode in (True, False):
        enc.train(mode)
        dec.train(mode)
        for _ in range(STEPS):
            z = enc(x)
            z.square().sum().backward()
            x_hat = dec(z.detach())
            torch.nn.functional.mse_loss(x_hat, x).backward()
    return _digest([engine_for(enc), engine_for(dec)])


def fp8_128x256():
    """quant = 1 on 128 x 256 images (the module shells are square: this case binds its own arenas to a context)."""
    import torch
    from eae_amd import _lib
    lib = _lib.load()
    B = 2
    cfg = _lib.EaeConfig(64, 10, 128, 256, B, 1, 0, 3)
    poff, boff = (C.c_longlong * 39)(), (C.c_longlong * 15)()
    _lib.check(lib.eae_ae_layout(C.byref(cfg), poff, boff))
    g = torch.Generator(device="cpu").manual_seed(7)

    class E:
        pass
    e = E()
    e.params = ((torch.rand(poff[38], generator=g) - 0.5) * 0.05).cuda()
    for gi, c in zip((2, 6, 10, 14, 22, 26, 30), (32, 64, 128, 256, 128, 64, 32)):
        e.params[poff[gi]: poff[gi] + c] = 1.0
    e.grads, e.adam_m, e.adam_v = (torch.zeros(poff[38], device="cuda") for _ in range(3))
    e.bn_running = torch.zeros(boff[14], device="cuda")
    for l, c in enumerate((32, 64, 128, 256, 128, 64, 32)):
        e.bn_running[boff[2 * l + 1]: boff[2 * l + 1] + c] = 1.0
    e.bn_nbt = torch.zeros(7, dtype=torch.int64, device="cuda")
    e.loss_accum, e.loss_last = torch.zeros(8, device="cuda"), torch.zeros(4, device="cuda")
    x = torch.rand((B, 3, 128, 256), generator=g).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    ctx = C.c_void_p()
    _lib.check(lib.eae_create(C.byref(cfg), C.byref(ctx)))
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.eae_bind(ctx, p(e.params), p(e.grads), p(e.adam_m), p(e.adam_v), p(e.bn_running), p(e.bn_nbt)))
    io = _lib.EaeStepIO(p(x), p(y), B, 1, 1, ALPHA, None, None, None, p(e.loss_accum), p(e.loss_last))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.eae_fp8_calibrate(ctx, st, C.byref(io), 7))
    for _ in range(STEPS):
        _lib.check(lib.eae_ae_train_step(ctx, st, C.byref(io), LR))
    d = _digest([e])
    _lib.check(lib.eae_destroy(ctx))
    return d


def _wce(eng):
    eng.set_class_weights([0.5, 2.0, 1.0, 1.0, 3.0, 0.25, 1.0, 1.0, 1.5, 1.0], ignore_index=-100)


# name -> (environment of the process, function)
CASES = {
    "b2": ({}, lambda: train(2)),
    "b8": ({}, lambda: train(8)),
    "b130": ({}, lambda: train(130)),                     # crosses the 128-row tile of the masked projection
    "latent48": ({}, lambda: train(8, latent=48)),        # the padded gradient shadows
    "bands1": ({}, lambda: train(2, bands=1)),
    "bands16": ({}, lambda: train(2, bands=16)),
    "img256": ({}, lambda: train(2, size=256)),           # split-K ranges of the latent projections longer than 128
    "fp8_128x256": ({}, fp8_128x256),
    "nohead": ({}, lambda: train(8, head=False)),
    "wce_ignore": ({}, lambda: train(8, setup=_wce)),
    "clip": ({}, lambda: train(8, setup=lambda e: e.set_grad_clip(0.5))),
    "autograd_train": ({}, lambda: autograd(True)),       # eae_ae_forward + eae_ae_backward
    "autograd_eval": ({}, lambda: autograd(False)),
    "halves": ({}, halves),                               # encoder alone, decoder alone: forward + backward, train and eval mode
    "split_step": ({}, split_step),                       # eae_ae_grad_step_begin / _end
    "group3": ({}, group3),
    "b8_no_fold_fwd": ({"EAE_NO_FOLD_FWD": "1"}, lambda: train(8)),
    "b8_no_fold_bwd": ({"EAE_NO_FOLD_BWD": "1"}, lambda: train(8)),
    "b8_fork_events": ({"EAE_FORK_EVENTS": "1"}, lambda: train(8)),
    "b8_no_side_stream": ({"EAE_NO_SIDE_STREAM": "1"}, lambda: train(8)),
    "b8_side_streams_1": ({"EAE_SIDE_STREAMS": "1"}, lambda: train(8)),
    "b8_dy_mask_clear": ({"EAE_DY_MASK": "0"}, lambda: train(8)),
    "b8_dy_mask_all": ({"EAE_DY_MASK": "0x3c"}, lambda: train(8)),
    "b8_graph_on": ({"EAE_GRAPH": "1"}, lambda: train(8)),
    "b8_graph_off": ({}, lambda: train(8, graph=False)),
}


def main(argv):
    if argv == ["--list"]:
        print("\n".join(CASES))
        return 0
    if argv[:1] == ["--all"] and all(n in CASES for n in argv[1:]):
        for name in argv[1:] or CASES:
            env = CASES[name][0]
            r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env={**os.environ, **env}, capture_output=True,
                               text=True, timeout=180)
            if r.returncode != 0:                         # nothing more is started on the device after a failure
                print(f"{name} FAILED ({r.returncode})\n{r.stdout}{r.stderr}", flush=True)
                return 1
            print(r.stdout.strip().splitlines()[-1], flush=True)
        return 0
    if len(argv) != 1 or argv[0] not in CASES:
        print(__doc__)
        return 2
    env, fn = CASES[argv[0]]
    missing = {k: v for k, v in env.items() if os.environ.get(k) != v}
    if missing:
        raise SystemExit(f"case {argv[0]} needs {missing} in the environment (--all sets it)")
    print(argv[0], fn(), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
