#!/usr/bin/env python3
"""Pins of the CPU oracle and the mirrored modules, produced by running the REFERENCE itself (imported, as make_golden.py does):
    FACEOFF_REFERENCE=<checkout of the reference> python tests/golden/make_golden_pins.py
writes
  ref_pins.npz                  VQVAE.forward + backward of one 3-frame clip at 32x48 (tests/test_oracle_vs_reference.py): outputs, codes, loss
                                and gradients (the same in train and eval mode, stored once) and the EMA buffers after the train-mode step
  ref_perturb_draws.json        perturb_image_composite's calls for seeds 0..199 with cv2 / wand / torchvision replaced by recorders
  ref_vqvae_checkpoint.pt.gz    a checkpoint written by the reference's VQVAE(in_channel=6): tensor i of its state_dict filled with i
                                (so that the file compresses and every value names the key it was saved under)
  ref_host.json                 the names of the functions utils.py defines (tests/test_dropin_cpu.py) and what the reference's
                                CycleScheduler returns and leaves in the param groups step by step (tests/test_host_cpu.py)
Data only: nothing from the reference's source is stored."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["FACEOFF_REFERENCE"]
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from faceoff_amd.synth import make_state_dict, make_batch  # noqa: E402
from make_golden import sub, stats  # noqa: E402


def literal(train):
    from models.vqvae_conv3d_latent import VQVAE
    torch.manual_seed(0)
    sd = make_state_dict(21, codebook_scale=0.3, gain=2.0)
    img, gt = make_batch(22, 1, 3, 32, 48)
    x, y = torch.from_numpy(img), torch.from_numpy(gt).reshape(3, 3, 32, 48)
    m = VQVAE(in_channel=6)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m.train(train)
    ids = {}
    m.quantize_t.register_forward_hook(lambda mod, a, o: ids.__setitem__("t", o[2]))
    m.quantize_b.register_forward_hook(lambda mod, a, o: ids.__setitem__("b", o[2]))
    dec, diff = m(x.reshape(3, 6, 32, 48))
    loss = torch.nn.functional.mse_loss(dec[:, :3], y) + diff.mean()
    loss.backward()
    res = {"dec": dec.detach().numpy(), "id_t": ids["t"].numpy().astype(np.int16), "id_b": ids["b"].numpy().astype(np.int16),
           "loss": np.float64(loss.item()),
           "grad_stats": np.stack([stats(p.grad) for _, p in m.named_parameters()]),
           "grad_sub": np.concatenate([sub(p.grad) for _, p in m.named_parameters()]),
           "param_names": np.array([k for k, _ in m.named_parameters()])}
    bufs = {k: b.detach().clone() for k, b in m.named_buffers()}
    return res, bufs


BUF_SUB = 7       # strided sample of the EMA buffers


def buffer_pins(bufs, ids):
    """cluster_size whole; embed / embed_avg [64, 512]: the columns of the codes the step used whole (the step's own update), every
    BUF_SUB-th entry and (sum, sum of squares, max |x|) of all of them"""
    out = {}
    for k, b in bufs.items():
        lvl = k.split(".")[0][-1]                    # quantize_t / quantize_b
        if k.endswith("cluster_size"):
            out["buf." + k] = b.numpy()
            continue
        cols = np.unique(ids[lvl]).astype(np.int64)
        out["buf_cols." + k] = cols
        out["buf_used." + k] = b[:, cols].numpy()
        out["buf_sub." + k] = sub(b, BUF_SUB)
        out["buf_stats." + k] = stats(b)
    return out


PERTURB_PROG = r'''
import sys, types, json, random
sys.path.insert(0, %r)
class _Img:
    def __enter__(self): return self
    def __exit__(self, *a): return False
    def distort(self, kind, args): CALLS.append(["distort_image", [TYPE[0], list(args[1:]) if kind != "arc" else list(args)], kind])
    def resize(self, *a): pass
    def __array__(self, *a, **k):
        import numpy as np
        return np.zeros((4, 4, 3), np.uint8)
for name in ("cv2", "wand", "wand.image", "torchvision", "torchvision.transforms", "matplotlib", "matplotlib.pyplot", "PIL", "PIL.Image"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["wand.image"].Image = types.SimpleNamespace(from_array=lambda a: _Img())
sys.modules["PIL"].Image = sys.modules["PIL.Image"]
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
import numpy as np
import TemporalAlignment.perturbations as R
CALLS, TYPE = [], [None]
def rec(name):
    def f(v, image, **kw):
        CALLS.append([name, v]); return image
    return f
real_distort = R.distort_image
def distort(t, image):
    TYPE[0] = t
    return real_distort(t, image)
for n in ("translate_horizontal", "translate_vertical", "rotate_image", "resize_image"):
    setattr(R, n, rec(n))
R.distort_image = distort
R.find_eye_center = lambda lm: (1.0, 2.0)
out = []
for seed in range(200):
    random.seed(seed); del CALLS[:]
    _, gt = R.perturb_image_composite(np.zeros((4, 4, 3), np.uint8), None)
    out.append({"calls": [c[:2] for c in CALLS], "kinds": [c[2] for c in CALLS if len(c) > 2], "gt": gt, "next": random.random()})
print(json.dumps(out))
'''


def perturb_draws():
    res = subprocess.run([sys.executable, "-c", PERTURB_PROG % REF], capture_output=True, text=True, cwd=HERE, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def checkpoint(path):
    from models.vqvae_conv3d_latent import VQVAE
    m = VQVAE(in_channel=6)
    with torch.no_grad():
        for i, v in enumerate(m.state_dict().values()):
            v.fill_(i)
    tmp = path + ".tmp"
    torch.save(m.state_dict(), tmp)
    with open(tmp, "rb") as src, gzip.GzipFile(path, "wb", mtime=0) as dst:
        dst.write(src.read())
    os.remove(tmp)


def host():
    import ast
    import importlib.util
    names = [n.name for n in ast.parse(open(os.path.join(REF, "utils.py")).read()).body if isinstance(n, ast.FunctionDef)]
    spec = importlib.util.spec_from_file_location("ref_scheduler", os.path.join(REF, "scheduler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    class Opt:
        param_groups = [{"lr": 0.0}]
    r = mod.CycleScheduler(Opt(), 3e-4, n_iter=200, momentum=None, warmup_proportion=0.05)
    cosine = [r.step()[0] for _ in range(200)]
    defaults = []                      # default arguments (momentum cycling, 30 % warm-up) over two and a half cycles
    for groups in ([{"lr": 0.0, "betas": (0.9, 0.999)}], [{"lr": 0.0, "momentum": 0.9}]):
        class B:
            param_groups = [dict(g) for g in groups]
        r = mod.CycleScheduler(B(), 1e-3, n_iter=37)
        defaults.append({"groups": groups, "steps": [[list(r.step()), [dict(g) for g in B.param_groups]] for _ in range(93)]})
    return {"utils_functions": names, "scheduler_warmup_cosine": cosine, "scheduler_defaults": defaults}


if __name__ == "__main__":
    pins, bufs = literal(True)
    pins_eval, bufs_eval = literal(False)
    assert pins.keys() == pins_eval.keys() and all(np.array_equal(pins[k], pins_eval[k]) for k in pins)      # one copy serves both modes
    pins.update(buffer_pins(bufs, {"t": pins["id_t"], "b": pins["id_b"]}))
    np.savez_compressed(os.path.join(HERE, "ref_pins.npz"), **pins)
    with open(os.path.join(HERE, "ref_perturb_draws.json"), "w") as fh:
        json.dump(perturb_draws(), fh, separators=(",", ":"))
    checkpoint(os.path.join(HERE, "ref_vqvae_checkpoint.pt.gz"))
    with open(os.path.join(HERE, "ref_host.json"), "w") as fh:
        json.dump(host(), fh, indent=0)
    print({f: os.path.getsize(os.path.join(HERE, f)) for f in ("ref_pins.npz", "ref_perturb_draws.json", "ref_vqvae_checkpoint.pt.gz", "ref_host.json")})
