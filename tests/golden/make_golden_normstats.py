"""Generates tests/golden/g20_normstats.npz by running the REFERENCE's own normalisation code on CPU torch, in fp32 and on the
same values widened to fp64.  Run by hand where the reference is available; the tests only read the .npz.

What is reference code here (loaded by file path from the reference tree, nothing re-typed):
  * `utils/stats.py::RunningStats`, `datasets/bases.py::global_contrast_normalization` and
    `TorchvisionDataset._update_transforms` ITSELF, on an instance made with `object.__new__` over a raw set of (image, label,
    index) triples; its `DataLoader(batch_size=2, shuffle=False, num_workers=4)` is the stock loader with the worker count set to
    0 (same batches, no subprocesses), and `transforms.Normalize` / `transforms.Compose` are recording stand-ins (torchvision is
    absent);
  * `utils/transformations.py::GlobalContrastNormalization` (in place, as the trainer calls it on the device);
  * the trajectory: `models/cnn.py::CNN32(bias=True)`, `training/hsc.py::HSCTrainer.loss / compute_anomaly_score`, stock Adam.
torchvision's `Normalize` (absent) is stood in for by its one line, (x - mean[:, None, None]) / std[:, None, None] in the dtype
of x.

Every case is stored twice: the reference in fp32 and the same code on the same fp32 values widened to fp64 ("64" keys).  The
distance between the two is the reference's own rounding noise; it is stored ("noise/...") and asserted to be non-zero, since
the tests allow K_NOISE_PARITY times it.

Inputs are pure functions of a name (oracle.fill), so the fixture holds only results:
  statistics  uint8 NHWC sets: ramp37 (37 x 32 x 32 x 3, a brightness ramp over the set: odd count, and the mean of batch means
              is visibly not the plain mean -- asserted), gray40 (40 x 28 x 28 x 1), rect9 (9 x 64 x 48 x 3), ramp37 restricted to
              an ascending list of 20 rows (pairs form over the LISTED images); both modes each.
  operator    fill(std 0.25, mean 0.5): [6, 3, 32, 32], [5, 1, 28, 28], [2, 3, 224, 224] (stored on the grid [::8, ::8]); scale l1
              and l2; with and without Normalize([tmin] * C, [tmax - tmin] * C).  The fp64 twins are stored in full (random
              doubles do not compress: 0.85 MB of the file), the fp32 outputs for the 28 x 28 and 224 cases; those of [6, 3, 32, 32]
              (0.3 MB more) would put the file over the 1 MiB limit for committed files.  What the tests need of the fp32 run
              is its distance to the twin, which is stored for every case.
  trajectory  K = 10 steps, 16 + 16 images of 32 x 32 in [0, 1], each batch through GCN + Normalize(ramp37's tmin / tmax) first.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
from oracle import models as omodels   # noqa: E402
from normstats_util import (OP_SHAPES, STATS_CASES, TRAJ_STEPS, op_input, stats_index, stats_set,   # noqa: E402
                            traj_batch)    # the inputs: pure functions of a name, shared with the tests

REF = "/root/reference/src/eoe"
sys.path.insert(0, "/root/reference/src")


# ------------------------------------------------------------------------------------------------ the reference, loaded by path
def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    if "." in name:
        parent, leaf = name.rsplit(".", 1)
        if parent in sys.modules:
            setattr(sys.modules[parent], leaf, m)
    return m


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


class RecNormalize:
    """records what `transforms.Normalize(mean, std, inplace=False)` was built with, and applies torchvision's one line"""

    def __init__(self, mean, std, inplace=False):
        self.mean, self.std = mean, std

    def __call__(self, x):
        m = torch.as_tensor(self.mean, dtype=x.dtype).view(-1, 1, 1)
        s = torch.as_tensor(self.std, dtype=x.dtype).view(-1, 1, 1)
        return (x - m) / s


class RecCompose:
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


def load_reference():
    _stub("torchvision").__path__ = []
    _stub("torchvision.transforms", Compose=RecCompose, Normalize=RecNormalize, Grayscale=type("Grayscale", (), {})).__path__ = []
    _stub("torchvision.transforms.functional", to_tensor=None, to_pil_image=None)
    _stub("torchvision.datasets", VisionDataset=object)
    _stub("torchvision.models", wide_resnet50_2=None)
    _stub("kornia").__path__ = []
    _stub("kornia.filters", gaussian_blur2d=None)
    _stub("eoe.utils.logger", Logger=object)
    _stub("eoe.datasets", str_labels=None).__path__ = []
    _stub("eoe.training").__path__ = []
    _stub("eoe.training.ad_trainer", ADTrainer=type("ADTrainer", (), {}))
    _stub("eoe.models.clip_official").__path__ = []
    _stub("eoe.models.clip_official.clip")
    np.infty = np.inf                                                   # bases.py uses the numpy < 2 alias
    stats = _load("eoe.utils.stats", f"{REF}/utils/stats.py")
    trf = _load("eoe.utils.transformations", f"{REF}/utils/transformations.py")
    bases = _load("eoe.datasets.bases", f"{REF}/datasets/bases.py")
    stock = torch.utils.data.DataLoader
    # the reference's loader call with the workers switched off: same batches of two in dataset order, no subprocesses
    bases.DataLoader = lambda dataset, **kw: stock(dataset, **{**kw, "num_workers": 0, "pin_memory": False})
    bases.tqdm = lambda it, **kw: it
    hsc = _load("eoe.training.hsc", f"{REF}/training/hsc.py")
    from eoe.models.cnn import CNN32
    return stats, trf, bases, hsc, CNN32


class RawSet(torch.utils.data.Dataset):
    """the raw training split `_update_transforms` walks: ToTensor'd images (u8 / 255 in fp32; the twin widens THOSE values)"""

    def __init__(self, u8_nhwc: np.ndarray, dtype):
        x = torch.from_numpy(u8_nhwc).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
        self.x = x.to(dtype)

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i].clone(), 0, i


class _Log:
    def print(self, *a, **k):
        pass


def ref_update_transforms(bases, u8, mode_str, dtype):
    """the reference's `_update_transforms` on a bare instance; returns (statistics dict, the installed transform)"""
    # the class is abstract in one loader hook that `_update_transforms` never calls: a subclass that only fills that in
    bare = type("BareDataset", (bases.TorchvisionDataset,), {"_get_raw_train_set": lambda self: None})
    ds = object.__new__(bare)
    ds.train_transform, ds.test_transform = RecCompose([mode_str]), RecCompose([mode_str])
    ds.logger, ds.normal_classes, ds.root = _Log(), [0], None
    stats = ds._update_transforms(RawSet(u8, dtype), cache=False, load=None)
    assert ds.train_transform.transforms[0] is ds.test_transform.transforms[0]
    return stats, ds.train_transform.transforms[0]


def main():
    RunningStatsMod, T, bases, hsc, RefCNN32 = load_reference()
    torch.set_num_threads(8)
    out = {}
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) /       # noqa: E731
                                    np.maximum(1e-300, np.abs(np.asarray(b, np.float64)))))

    # ---- statistics
    fitted = {}
    for case in STATS_CASES:
        set_name, idx = stats_index(case)
        u8 = stats_set(set_name)
        if idx is not None:
            u8 = u8[idx]
            out[f"stats/{case}/index"] = idx
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            st, norm = ref_update_transforms(bases, u8, "normalize", dt)
            assert st["mode"] == 0 and isinstance(norm, RecNormalize)
            out[f"stats/{case}/mean{tag}"] = st["mean"].double().numpy()
            out[f"stats/{case}/std{tag}"] = st["std"].double().numpy()
            st, norm = ref_update_transforms(bases, u8, "gcn-normalize", dt)
            assert st["mode"] == 1 and isinstance(norm.transforms[0], T.GlobalContrastNormalization) and norm.transforms[0].scale == "l1"
            tmin, rng = st["mean"][0], st["std"][0]
            assert st["mean"] == [tmin] * u8.shape[3] and st["std"] == [rng] * u8.shape[3]
            out[f"stats/{case}/tmin{tag}"], out[f"stats/{case}/tmax{tag}"] = np.float64(tmin), np.float64(tmin + rng)
            out[f"stats/{case}/range{tag}"] = np.float64(rng)
            fitted[(case, tag)] = (tmin, rng)
        for k in ("mean", "std", "tmin", "tmax", "range"):
            n = rel(out[f"stats/{case}/{k}32"], out[f"stats/{case}/{k}64"])
            assert n > 0.0, (case, k)
            out[f"noise/stats/{case}/{k}"] = np.float64(n)
        print(case, {k: f"{out[f'noise/stats/{case}/{k}']:.2e}" for k in ("mean", "std", "tmin", "tmax", "range")})
    # the batch-mean weighting is visible on the ramp: a textbook reduction cannot meet this case
    plain = stats_set("ramp37").astype(np.float64).mean(axis=(0, 1, 2)) / 255.0
    gap = np.abs(out["stats/ramp37/mean64"] - plain).max()
    assert gap > 1e-3, gap
    out["stats/ramp37/plain_mean"] = plain
    print(f"ramp37: reference mean {out['stats/ramp37/mean64']} plain mean {plain} (gap {gap:.2e})")

    # ---- operator
    tmin, rng = fitted[("ramp37", "64")]
    out["op/shift"], out["op/range"] = np.float64(tmin), np.float64(rng)
    for size in OP_SHAPES:
        x32 = op_input(size)
        C = x32.shape[1]
        for scale in ("l1", "l2"):
            for affine in (0, 1):
                res = {}
                for tag, dt in (("32", torch.float32), ("64", torch.float64)):
                    x = torch.from_numpy(x32.copy()).to(dt)          # GCN works in place: never on the shared input
                    y = T.GlobalContrastNormalization(scale=scale)(x)
                    assert y is x                                                   # in place, returns its argument
                    if affine:
                        y = T.Normalize(RecNormalize([tmin] * C, [rng] * C))(y)
                    y = y.double().numpy()
                    res[tag] = y[:, :, ::8, ::8] if size == "224" else y
                    if tag == "64":
                        out[f"op/{size}/{scale}/{affine}/y64"] = res[tag]
                    elif size != "32":              # the fp32 outputs where they fit (as g17 does): the 1 MiB file limit
                        out[f"op/{size}/{scale}/{affine}/y32"] = res[tag].astype(np.float32)
                n = float((np.abs(res["32"] - res["64"]) / np.maximum(1.0, np.abs(res["64"]))).max())
                assert n > 0.0
                out[f"noise/op/{size}/{scale}/{affine}"] = np.float64(n)
                print(f"op {size} {scale} affine={affine}: noise {n:.2e}, |y| max {np.abs(res['64']).max():.2f}")

    # ---- trajectory
    HSC = object.__new__(hsc.HSCTrainer)
    HSC.__dict__.update(device=torch.device("cpu"))
    res = {}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        torch.manual_seed(0)
        model = omodels.deterministic_init(RefCNN32(bias=True), tag="cnn32").to(dt).train()
        gcn = T.GlobalContrastNormalization(scale="l1")
        norm = T.Normalize(RecNormalize([tmin] * 3, [rng] * 3))
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.0, amsgrad=False)
        losses, scores = [], []
        for i in range(TRAJ_STEPS):
            x, y = traj_batch(i)
            imgs, lbls = norm(gcn(torch.from_numpy(x).to(dt))), torch.from_numpy(y)
            opt.zero_grad()
            feats = model(imgs)
            loss = HSC.loss(feats, lbls, None, nominal_label=0)
            loss.backward()
            opt.step()
            opt.zero_grad()
            losses.append(loss.item())
            scores.append(HSC.compute_anomaly_score(feats.detach(), None, nominal_label=0).double().numpy().copy())
        res[tag] = (np.array(losses, np.float64), np.stack(scores))
    out["traj/losses"], out["traj/scores"] = res["32"][0], res["32"][1].astype(np.float32)
    out["traj/losses64"], out["traj/scores64"] = res["64"]
    assert np.abs(res["32"][0] - res["64"][0]).max() > 0.0
    print("trajectory losses", res["32"][0], "noise", np.abs(res["32"][0] - res["64"][0]).max(), "scores",
          np.abs(res["32"][1] - res["64"][1]).max())

    path = os.path.join(HERE, "g20_normstats.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
