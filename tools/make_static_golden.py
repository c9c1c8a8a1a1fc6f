#!/usr/bin/env python3
"""Generate tests/golden/static_pad4d.npz by running the REFERENCE's own pre-processing with static attributes.

    python tools/make_static_golden.py --reference <checkout of the reference project>

The reference's dataset.py imports xarray and torchvision, which are not needed for the path pinned here, so both are
stubbed: ``xr.open_dataset`` returns an object whose ``data_vars`` hold seeded (H, W) f32 fields plus one ``lai_*``
variable that the reference skips (dataset.py:104-109).  ``E33OMA90D_CRNN.__getitem__`` (dataset.py:618-630) then runs on
an object built with ``__new__`` that holds one seeded, already z-scored window: it appends the static attributes
(z-scored over space, repeated over T, dataset.py:100-122) after the five dynamic channels and pads with the RNN pad
(dataset.py:67-98, the np.fliplr channel-flip quirk included).

Each case stores the window, the raw static fields S and the reference's padded X.  Only the .npz (data) is kept in the
repository; the reference source is read when this script runs and never copied.  Output is deterministic (seeded
arrays, fixed zip timestamps), so a rerun reproduces the file bit for bit."""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "static_pad4d.npz")

# (name, S, T, (H, W), (Hp, Wp), seed): S = 3 is the reference launcher's --in-channels 8, S = 16 the number of non-lai
# variables of the notebook that builds static_attrs.nc
CASES = [("s3", 3, 4, (12, 16), (16, 22), 31), ("s16", 16, 3, (12, 16), (16, 22), 32)]


def static_vars(S, H, W, seed):
    """S seeded non-constant f32 fields, each on its own scale, with one lai_* variable in the middle (skipped)"""
    rng = np.random.default_rng(seed)
    out = {}
    for i in range(S):
        if i == S // 2:
            out["lai_mean"] = rng.standard_normal((H, W)).astype(np.float32)
        scale, off = 10.0 ** rng.uniform(-2, 2), rng.uniform(-5, 5)
        out[f"attr{i:02d}"] = (off + scale * rng.standard_normal((H, W))).astype(np.float32)
    return out


def load_reference_dataset(ref_dir):
    fake_xr = types.ModuleType("xarray")
    fake_xr.open_dataset = lambda *a, **k: fake_xr._current          # add_static_attributes: xr.open_dataset(path)
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tv.transforms = tvt
    sys.modules.update({"xarray": fake_xr, "torchvision": tv, "torchvision.transforms": tvt})
    spec = importlib.util.spec_from_file_location("ref_dataset", os.path.join(ref_dir, "dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, fake_xr


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="directory holding the reference's dataset.py")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    ref, fake_xr = load_reference_dataset(args.reference)
    arrs = {}
    for name, S, T, (H, W), (Hp, Wp), seed in CASES:
        rng = np.random.default_rng(seed + 1000)
        window = rng.standard_normal((T, 5, H, W)).astype(np.float32)    # self.X[index]: already z-scored (dataset.py:593)
        dv = static_vars(S, H, W, seed)
        fake_xr._current = types.SimpleNamespace(data_vars=dv)
        ds = ref.E33OMA90D_CRNN.__new__(ref.E33OMA90D_CRNN)
        ds.period, ds.species, ds.padding, ds.seq_len, ds.in_channels = "train", "bcb", (Hp, Wp), T, 5 + S
        ds.X = window[None]
        ds.y = np.zeros((1, H, W), dtype=np.float32)
        X, _ = ds[0]
        X = X.numpy()
        assert X.shape == (T, 5 + S, Hp, Wp) and X.dtype == np.float32, X.shape
        arrs[f"{name}.window"] = window
        arrs[f"{name}.S"] = np.stack([v for k, v in dv.items() if not k.startswith("lai")])
        arrs[f"{name}.X"] = X
        arrs[f"{name}.padding"] = np.array([Hp, Wp], dtype=np.int32)
    arrs["note"] = np.array("reference E33OMA90D_CRNN.__getitem__ with static attributes (dataset.py:100-122, 618-630), "
                            "xarray / torchvision stubbed; window = the z-scored self.X[index], S = the raw non-lai fields")
    np.savez_compressed(args.out, **arrs)
    print(f"{args.out}: {os.path.getsize(args.out) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
