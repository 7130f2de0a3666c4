"""Golden-vector generator for the submission input path (SpeedSubmission,
REV/datasets/speed.py:44-160).  Runs only where a checkout of the reference exists; no test reads
the reference, only the fixture this writes.

REV/datasets/speed.py imports packages absent here (cv2, albumentations, torchvision) and its own
utils.speed_eval.  As oracle/gen_golden_solver_front.py does, it is imported with stand-ins for
them: cv2 carries the INTER_CUBIC constant, A.Resize is backed by the restated 8-bit cubic resize
(oracle/preprocess_ref.py resize_cubic_u8), F.to_tensor / F.normalize by torchvision's arithmetic
in numpy float32.  Everything the fixture pins is then the reference's own code: load_anns,
generate_clip_bbox (the integer square), the canvas and the copy of __getitem__, run through the
real SpeedSubmission over grayscale JPEG files in a temporary DATA_ROOT.

Frames.  Cases on SPEED's 1920x1200 frame (the boxes taken from the reference's test-set detector
results, annos/wz_real_test.json and wz_synt_test.json) share one frame that is constant over
every 8x8 block: with an all-ones quantisation table its JPEG round trip is exact (asserted), so
the fixture stores the seed only.  Cases on small frames store the decoded frames themselves.

Writes tests/golden/submission_front_ref.npz:
  size                       S (32)
  big_seed, big_shape        the shared 1920x1200 frame: big_frame(seed) below
  small_frames [N,64,80]     decoded small frames (uint8)
  frame_index [K]            -1: the big frame, else an index into small_frames
  filenames [K], bbox [K,4]  the annotation entries (fp64 boxes)
  clip_bbox [K,4] int64      the reference's target["clip_bbox"]
  crops [K,S,S,3] uint8      the resized canvas (A.Resize's output)
  images [K,3,S,S] fp32      the normalised tensor __getitem__ returns
Usage: python scripts/gen_golden_submission.py --reference <path to the reference checkout>
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
REV_DIR = "Revisiting Monocular Satellite Pose Estimation With Transformer"
S = 32
SMALL = (64, 80)            # height, width
BIG = (1200, 1920)
BIG_SEED = 20201214

# (filename, file) picked from the reference's detector results: boxes whose square crosses the
# bottom, top, left + bottom, left + top + bottom edges, and interior ones
REAL = [("img000424real.jpg", "wz_real_test.json"), ("img000125real.jpg", "wz_real_test.json"),
        ("img000367real.jpg", "wz_real_test.json"), ("img000379real.jpg", "wz_real_test.json"),
        ("img000088real.jpg", "wz_real_test.json"), ("img006587.jpg", "wz_synt_test.json"),
        ("img012766.jpg", "wz_synt_test.json"), ("img005789.jpg", "wz_synt_test.json")]

# hand-written boxes on the small frame (width 80, height 64)
HAND = [
    ("left_trunc.jpg", [-6.3, 20.0, 13.7, 38.0]),       # xc - s/2 = -8.3 -> x1 = -8 (floor would give -9)
    ("top.jpg", [30.0, -4.5, 52.0, 15.5]),              # y1 = int(-7.7) = -7
    ("right.jpg", [58.0, 22.0, 84.0, 40.0]),            # x1 + side = 86 > 80
    ("bottom.jpg", [20.0, 44.0, 40.0, 70.0]),           # y1 + side = 72 > 64
    ("corner.jpg", [60.25, 45.5, 83.0, 66.75]),         # right + bottom
    ("interior.jpg", [22.4, 18.9, 47.1, 39.3]),
    ("side_eq_S.jpg", [20.0, 14.0, 47.0, 36.0]),        # int(27 * 1.2) = 32 = S: cv::resize copies
    ("tiny.jpg", [40.2, 30.1, 46.9, 35.0]),             # side 8: upscaling
    ("larger_than_frame.jpg", [-10.0, -5.0, 95.0, 70.0]),   # side 126: pad on all four sides
]


def big_frame(seed=BIG_SEED, shape=BIG):
    """uint8 frame constant over every 8x8 block, values in [16, 240)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = rng.integers(16, 240, (shape[0] // 8, shape[1] // 8), dtype=np.uint8)
    return np.kron(v, np.ones((8, 8), np.uint8))


def small_frame(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:SMALL[0], 0:SMALL[1]]
    g = 90 + 60 * np.sin(xx / 5.0 + seed) * np.cos(yy / 7.0) + rng.normal(0, 25, SMALL)
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


def _stand_ins():
    import preprocess_ref as pr
    import torch

    cv2 = types.ModuleType("cv2")
    cv2.INTER_CUBIC, cv2.BORDER_CONSTANT = 2, 0
    cv2.error = type("error", (Exception,), {})
    sys.modules["cv2"] = cv2

    alb = types.ModuleType("albumentations")

    class Resize:
        def __init__(self, height, width, interpolation):
            assert height == width and interpolation == cv2.INTER_CUBIC
            self.size = height

        def __call__(self, image):
            return pr.resize_cubic_u8(image, self.size)

    class Compose:
        def __init__(self, transforms, **kw):
            self.transforms = transforms

        def __call__(self, image):
            REC["canvas"].append(image.copy())
            for t in self.transforms:
                image = t(image)
            REC["resized"].append(image.copy())
            return {"image": image}

    alb.Resize, alb.Compose = Resize, Compose
    sys.modules["albumentations"] = alb

    tv = types.ModuleType("torchvision")
    tv.__path__ = []
    tvt = types.ModuleType("torchvision.transforms")
    tvt.__path__ = []
    tvf = types.ModuleType("torchvision.transforms.functional")

    def to_tensor(pic):                     # uint8 HWC -> float32 CHW / 255
        assert pic.dtype == np.uint8 and pic.ndim == 3
        return torch.from_numpy(pic.transpose(2, 0, 1).astype(np.float32) / np.float32(255))

    def normalize(tensor, mean, std):       # tensor.sub_(mean).div_(std), fp32
        m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
        s = torch.tensor(std, dtype=torch.float32)[:, None, None]
        return (tensor - m) / s

    tvf.to_tensor, tvf.normalize = to_tensor, normalize
    tv.transforms, tvt.functional = tvt, tvf
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})


REC = {"canvas": [], "resized": []}


def _import_speed(rev):
    """REV/datasets/speed.py under its own package name; its `from utils.speed_eval import
    speed_score` (unused by SpeedSubmission) gets an empty stand-in."""
    for k in [k for k in sys.modules if k in ("utils", "datasets") or k.startswith(("utils.", "datasets."))]:
        del sys.modules[k]
    u = types.ModuleType("utils")
    u.__path__ = []
    use = types.ModuleType("utils.speed_eval")
    use.speed_score = None
    d = types.ModuleType("datasets")
    d.__path__ = [os.path.join(rev, "datasets")]
    sys.modules.update({"utils": u, "utils.speed_eval": use, "datasets": d})
    spec = importlib.util.spec_from_file_location("datasets.speed", os.path.join(rev, "datasets", "speed.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["datasets.speed"] = m
    spec.loader.exec_module(m)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    rev = os.path.join(os.path.abspath(args.reference), REV_DIR)
    from PIL import Image

    anns, frame_index, small = {}, [], []
    for name, file in REAL:
        with open(os.path.join(rev, "annos", file)) as f:
            anns[name] = json.load(f)[name]
        frame_index.append(-1)
    for i, (name, box) in enumerate(HAND):
        anns[name] = [box + [1.0]]
        frame_index.append(i)
        small.append(small_frame(100 + i))

    _stand_ins()
    tmp = tempfile.mkdtemp()
    cwd = os.getcwd()
    try:
        root = os.path.join(tmp, "data", "speed")
        os.makedirs(os.path.join(root, "annos"))
        os.makedirs(os.path.join(root, "images"))
        with open(os.path.join(root, "annos", "det.json"), "w") as f:
            json.dump(anns, f)
        big = big_frame()
        ones = [1] * 64
        decoded_small = []
        for name, fi in zip(anns, frame_index):
            p = os.path.join(root, "images", name)
            if fi < 0:
                Image.fromarray(big).save(p, "JPEG", qtables=[ones])
                assert np.array_equal(np.asarray(Image.open(p)), big), "block-constant frame must round-trip"
            else:
                Image.fromarray(small[fi]).save(p, "JPEG", quality=92)
                decoded_small.append(np.asarray(Image.open(p)).copy())
        os.chdir(tmp)
        ds = _import_speed(rev)
        sub = ds.SpeedSubmission("det.json", "images", S)
        assert len(sub) == len(anns)
        clips, images, names = [], [], []
        for i in range(len(sub)):
            img, target = sub[i]
            names.append(target["filename"])
            clips.append(target["clip_bbox"].numpy().astype(np.int64))
            images.append(img.numpy())
            side = int(clips[-1][2] - clips[-1][0])
            assert REC["canvas"][i].shape == (side, side, 3)
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)

    assert names == list(anns)
    out = dict(size=np.int64(S), big_seed=np.int64(BIG_SEED), big_shape=np.asarray(BIG, np.int64),
               small_frames=np.stack(decoded_small), frame_index=np.asarray(frame_index, np.int64),
               filenames=np.asarray(names), bbox=np.asarray([anns[n][0][:4] for n in names], np.float64),
               clip_bbox=np.stack(clips), crops=np.stack(REC["resized"]), images=np.stack(images).astype(np.float32))
    path = os.path.join(REPO, "tests", "golden", "submission_front_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for n, c in zip(names, out["clip_bbox"]):
        print(f"  {n:28s} clip {c.tolist()} side {int(c[2] - c[0])}")


if __name__ == "__main__":
    main()
