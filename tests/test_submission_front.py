"""Submission input path (SpeedSubmission, REV/datasets/speed.py:44-160; gen_submission,
REV/gen_submission_single.py:113-187, gen_submission_multi.py:123-186).

CPU: the numpy restatement (tests/submission_ref.py) against the fixture recorded from the
reference's own SpeedSubmission (tests/golden/submission_front_ref.npz, written by
scripts/gen_golden_submission.py), the status rule, the pad region, and generate_submission's host
logic with stub decoder / transform / model / solver objects.
GPU: csrc/preprocess.hip's submission kernel against the restatement and the fixture, bit-exact
(uint8 crops, fp32 images, clip_bbox, status), its nullable outputs, the u8 model entry on its
crops, and generate_submission end to end from JPEG bytes.
"""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import preprocess_ref as pr
import submission_ref as sr
from conftest import GOLDEN


# ---------------------------------------------------------------------------------- fixture
@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(os.path.join(GOLDEN, "submission_front_ref.npz")))
    rng = np.random.Generator(np.random.PCG64(int(g["big_seed"])))
    h, w = (int(v) for v in g["big_shape"])
    big = np.kron(rng.integers(16, 240, (h // 8, w // 8), dtype=np.uint8), np.ones((8, 8), np.uint8))
    g["frames"] = [big if i < 0 else g["small_frames"][i] for i in g["frame_index"]]
    return g


def test_fixture_covers_the_edge_cases(golden):
    """The recorded boxes are the ones the checks below rely on: >= 12 boxes, >= 6 of the
    reference's test-set detector boxes, every frame edge crossed, a negative x1 that truncation
    towards zero and floor place differently, an interior box and one with side == S."""
    g = golden
    S = int(g["size"])
    clip = g["clip_bbox"]
    hw = np.array([f.shape for f in g["frames"]])
    assert len(clip) >= 12 and int((g["frame_index"] < 0).sum()) >= 6
    assert (clip[:, 0] < 0).any() and (clip[:, 1] < 0).any()
    assert (clip[:, 2] > hw[:, 1]).any() and (clip[:, 3] > hw[:, 0]).any()
    inside = (clip[:, 0] >= 0) & (clip[:, 1] >= 0) & (clip[:, 2] <= hw[:, 1]) & (clip[:, 3] <= hw[:, 0])
    assert inside.any() and (clip[:, 2] - clip[:, 0] == S).any()
    b = g["bbox"]
    s = np.maximum(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]) * 1.2
    x1f = (b[:, 0] + b[:, 2]) / 2 - s / 2
    assert ((x1f < 0) & (np.floor(x1f) != clip[:, 0])).any()


def test_restatement_matches_reference_fixture(golden):
    g = golden
    S = int(g["size"])
    for i, frame in enumerate(g["frames"]):
        o = sr.preprocess(frame[None], g["bbox"][i:i + 1], S)
        assert o["status"][0] == 0
        assert np.array_equal(o["clip_bbox"][0], g["clip_bbox"][i]), g["filenames"][i]
        # the reference converts to RGB before the crop: three equal channels
        assert np.array_equal(np.repeat(o["crops"][0][..., None], 3, -1), g["crops"][i]), g["filenames"][i]
        assert np.array_equal(o["images"][0], g["images"][i]), g["filenames"][i]


def test_generate_clip_bbox_submission_matches_fixture(golden):
    from spe.datasets import generate_clip_bbox_submission
    for b, c in zip(golden["bbox"], golden["clip_bbox"]):
        got = generate_clip_bbox_submission(b)
        assert got.dtype == np.int64 and np.array_equal(got, c)


def test_status_rule():
    """status 1: side <= 0, or no positive-area overlap with the frame (width 200, height 160)."""
    W, H = 200, 160

    def status(box):
        return int(sr.preprocess(np.full((1, H, W), 9, np.uint8), np.asarray([box], np.float64), 16)["status"][0])

    assert status([50.0, 50.0, 50.5, 50.5]) == 1                 # side = int(0.6) = 0
    assert status([50.0, 50.0, 40.0, 45.0]) == 1                 # negative extent: side < 0
    assert status([-60.0, 40.0, -40.0, 60.0]) == 1               # left of the frame
    assert status([230.0, 40.0, 250.0, 60.0]) == 1               # right
    assert status([40.0, -60.0, 60.0, -40.0]) == 1               # above
    assert status([40.0, 190.0, 60.0, 210.0]) == 1               # below
    # box [88, -23, 112, 1): exactly one frame row (y = 0) inside -> a crop; one row higher -> none
    assert sr.generate_clip_bbox([90.0, -21.0, 110.0, -1.0]).tolist() == [88, -23, 112, 1]
    assert status([90.0, -21.0, 110.0, -1.0]) == 0
    assert sr.generate_clip_bbox([90.0, -22.0, 110.0, -2.0]).tolist() == [88, -24, 112, 0]
    assert status([90.0, -22.0, 110.0, -2.0]) == 1
    # the same at the right edge: x1 = 199 shares column 199, x1 = 200 shares nothing
    assert sr.generate_clip_bbox([201.0, 40.0, 221.0, 60.0]).tolist()[0] == 199
    assert status([201.0, 40.0, 221.0, 60.0]) == 0
    assert status([202.0, 40.0, 222.0, 60.0]) == 1
    o = sr.preprocess(np.full((1, H, W), 9, np.uint8), np.asarray([[230.0, 40.0, 250.0, 60.0]]), 16)
    assert not o["images"].any() and not o["crops"].any()        # zeros, not the normalised zero


def test_pad_region_is_zero_and_inside_is_the_frame():
    """side == S, so the resize copies the canvas: outside the frame exactly 0, inside the frame."""
    rng = np.random.Generator(np.random.PCG64(8))
    frame = rng.integers(1, 256, (64, 80), dtype=np.uint8)       # no zero pixel inside
    S = 32
    for box in ([-9.0, -12.0, 18.0, 10.0], [60.0, 44.0, 87.0, 66.0]):
        o = sr.preprocess(frame[None], np.asarray([box]), S)
        x1, y1, x2, y2 = o["clip_bbox"][0]
        assert x2 - x1 == S and o["status"][0] == 0
        yy, xx = np.mgrid[y1:y2, x1:x2]
        inside = (xx >= 0) & (xx < 80) & (yy >= 0) & (yy < 64)
        assert inside.any() and (~inside).any()
        crop = o["crops"][0]
        assert (crop[~inside] == 0).all()
        assert np.array_equal(crop[inside], frame[yy[inside], xx[inside]])
        assert np.array_equal(o["images"][0], pr.to_tensor_normalize(crop))


# ------------------------------------------------------------- generate_submission, host logic
def _jpeg(a, **kw):
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "JPEG", **kw)
    return bio.getvalue()


class _Stubs:
    """Stand-ins on the CPU.  A file is either b"raw:<v>" (the stub decoder returns a frame filled
    with v) or a real JPEG the stub decoder refuses with status 1, like a progressive file."""
    H, W = 8, 16

    def __init__(self):
        self.transform_calls, self.single_calls, self.multi_calls = [], [], []

    def decoder(self, data, offsets, sizes):
        data, B = data.numpy().tobytes(), offsets.numel()
        frames = torch.zeros(B, self.H, self.W, dtype=torch.uint8)
        status = torch.zeros(B, dtype=torch.int32)
        for i, (o, n) in enumerate(zip(offsets.tolist(), sizes.tolist())):
            f = data[o:o + n]
            if f.startswith(b"raw:"):
                frames[i] = int(f[4:])
            else:
                status[i] = 1
        return {"frames": frames, "status": status}

    def transform(self, frames, bbox, crops=False, images=True):
        assert crops and not images
        self.transform_calls.append((frames.clone(), np.array(bbox)))
        bb = torch.as_tensor(bbox, dtype=torch.float32)
        return {"crops": frames, "clip_bbox": bb, "status": (bb[:, 0] < 0).to(torch.int32)}

    def model(self, scale):
        def forward(crops, clip_bbox=None):
            v = crops.reshape(crops.shape[0], -1).double().mean(1) * scale
            return {"points_px": v[:, None, None].float().expand(-1, 11, 2),
                    "probs": clip_bbox[:, :1, None].expand(-1, 11, 12)}
        return forward

    def _poses(self, v, probs):
        B = v.shape[0]
        quat = (v[:, None] + torch.tensor([0.12345649, 0.5000005, -0.9999996, 1e-7])).float()
        tvec = v[:, None].double() * torch.tensor([1.00000049, -2.0000005, 3.14159265358979], dtype=torch.float64)
        # probs carries x1 of the box: the stub solver fails (NO_FG, CV_ERROR, UNPINNED) or falls back on request
        status = torch.tensor([{11: 1, 12: 2, 13: 3, 14: 4}.get(int(x), 0) for x in probs[:, 0, 0].tolist()],
                              dtype=torch.int32)
        return {"quat": quat, "tvec": tvec, "status": status}

    def solve_batch(self, points_px, probs, sigmas=None):
        self.single_calls.append(points_px.shape[0])
        return self._poses(points_px[:, 0, 0].double(), probs)

    def solve_batch_multi(self, multi_points, multi_probs):
        self.multi_calls.append((len(multi_points), multi_points[0].shape[0]))
        return self._poses(torch.stack(list(multi_points)).double().mean(0)[:, 0, 0], multi_probs[0])


class _SingleSolver:
    def __init__(self, s):
        self.solve_batch = s.solve_batch


def _stub_run(models_of, solver_of, batch_size=2):
    from spe.engine import generate_submission
    s = _Stubs()
    rng = np.random.Generator(np.random.PCG64(2))
    gray = rng.integers(0, 256, (s.H, s.W), dtype=np.uint8)
    colour = rng.integers(0, 256, (s.H, s.W, 3), dtype=np.uint8)
    files = {"z_first.jpg": b"raw:40", "a_second.jpg": _jpeg(gray, progressive=True),
             "m_third.jpg": b"raw:7", "b_fourth.jpg": _jpeg(colour, quality=95),
             "k_fifth.jpg": b"raw:90", "c_nofg.jpg": b"raw:50", "d_cverr.jpg": b"raw:51",
             "e_fallback.jpg": b"raw:52", "f_unpinned.jpg": b"raw:53", "g_crop.jpg": b"raw:54",
             "h_last.jpg": b"raw:55"}
    x1 = {"c_nofg.jpg": 11.0, "d_cverr.jpg": 12.0, "e_fallback.jpg": 13.0, "f_unpinned.jpg": 14.0, "g_crop.jpg": -3.0}
    anns = {f: [[x1.get(f, 100.0 + i), 2.0, 30.0, 40.0, 0.99], [0.0, 0.0, 1.0, 1.0, 0.5]] for i, f in enumerate(files)}
    log = generate_submission(models_of(s), None, anns, files.__getitem__, solver_of(s), torch.device("cpu"),
                              batch_size, 8, decoder=s.decoder, transform=s.transform)
    return s, files, anns, log, gray, colour


def test_generate_submission_host_logic():
    s, files, anns, log, gray, colour = _stub_run(lambda s: s.model(1.0), lambda s: _SingleSolver(s))
    names = list(files)
    assert list(log) == names                                    # the mapping's order, not sorted
    assert s.single_calls == [2, 2, 2, 2, 2, 1] and not s.multi_calls   # drop_last=False: a short last batch
    # the first box of every file, fp64, in order
    assert np.array_equal(np.concatenate([b for _, b in s.transform_calls]),
                          np.asarray([anns[f][0][:4] for f in names], np.float64))
    # a refused gray file: decoded on the host, the batch stays 1-channel
    f0 = s.transform_calls[0][0]
    assert f0.shape == (2, s.H, s.W) and (f0[0] == 40).all()
    assert np.array_equal(f0[1].numpy(), np.asarray(Image.open(io.BytesIO(files["a_second.jpg"]))))
    # a colour file: the batch runs 3-channel, the gray frame replicated
    f1 = s.transform_calls[1][0]
    assert f1.shape == (2, s.H, s.W, 3) and (f1[0] == 7).all()
    assert np.array_equal(f1[1].numpy(), np.asarray(Image.open(io.BytesIO(files["b_fourth.jpg"])).convert("RGB")))
    assert all(f.dim() == 3 for f, _ in s.transform_calls[2:])
    # rounding: np.around(., 6) of the float32 quaternion as float64 and of the fp64 translation
    v = 40.0
    q = (torch.tensor([v], dtype=torch.float64)[:, None] + torch.tensor([0.12345649, 0.5000005, -0.9999996, 1e-7])).float()
    assert log["z_first.jpg"]["quat_pr"] == np.around(q[0].double().numpy(), 6).tolist()
    assert log["z_first.jpg"]["tvec_pr"] == np.around(v * np.array([1.00000049, -2.0000005, 3.14159265358979]), 6).tolist()
    assert log["z_first.jpg"]["tvec_pr"][2] == 125.663706
    # zero pose: solver status NO_FG / CV_ERROR / UNPINNED and a status-1 crop; RANSAC_FALLBACK keeps its pose
    for f in ("c_nofg.jpg", "d_cverr.jpg", "f_unpinned.jpg", "g_crop.jpg"):
        assert log[f] == {"quat_pr": [0.0] * 4, "tvec_pr": [0.0] * 3}, f
    assert log["e_fallback.jpg"]["tvec_pr"][0] == round(52 * 1.00000049, 6)
    assert all(isinstance(x, float) for r in log.values() for k in ("quat_pr", "tvec_pr") for x in r[k])
    assert all(set(r) == {"quat_pr", "tvec_pr"} for r in log.values())


def test_generate_submission_list_of_models_uses_the_ensemble_solver():
    s, files, anns, log, _, _ = _stub_run(lambda s: [s.model(1.0), s.model(3.0)], lambda s: s, batch_size=4)
    assert s.multi_calls == [(2, 4), (2, 4), (2, 3)] and not s.single_calls
    assert list(log) == list(files)
    assert log["k_fifth.jpg"]["tvec_pr"][0] == round(180 * 1.00000049, 6)     # mean of 90 and 270
    with pytest.raises(ValueError, match="ensemble solver"):
        _stub_run(lambda s: [s.model(1.0)], lambda s: _SingleSolver(s))


# ------------------------------------------------------------------------------------- GPU
def _case_boxes(H, W, S, with_empty):
    """The box kinds every configuration holds (name, box): interior, two corners (one with a
    negative fractional x1), tiny, larger than the frame, side == S, and optionally an off-frame
    (status 1) box."""
    w = (S + 0.3) / 1.2                                          # int(1.2 w) == S
    cases = [("interior", [0.3 * W, 0.3 * H, 0.3 * W + 0.21 * H + 0.4, 0.3 * H + 0.17 * H]),
             ("corner_br", [W - 0.2 * H, 0.8 * H + 0.5, W + 3.25, H + 6.0]),
             ("corner_tl", [-5.3, -2.0, 0.15 * H, 0.2 * H + 0.7]),
             ("tiny", [0.5 * W + 0.2, 0.5 * H + 0.1, 0.5 * W + 6.9, 0.5 * H + 5.0]),
             ("larger", [-0.1 * W, -0.2 * H, 1.1 * W, 1.15 * H]),
             ("side_eq_S", [0.25 * W - 0.5 * w, 0.4 * H - 0.3 * w, 0.25 * W + 0.5 * w, 0.4 * H + 0.3 * w])]
    if with_empty:
        cases.append(("empty", [W + 30.0, 50.0, W + 50.0, 70.0]))
    return cases


_REF = {}


def _reference(channels, H, W, S, B):
    """Frames, boxes (padded to a multiple of B with repeats) and the restatement's outputs, once."""
    key = (channels, H, W, S, B)
    if key not in _REF:
        cases = _case_boxes(H, W, S, with_empty=(H, W) == (160, 200))
        while len(cases) % B:
            cases.append(cases[len(cases) % 3])
        rng = np.random.Generator(np.random.PCG64(17 + S + channels))
        frames = rng.integers(0, 256, (B, H, W) + ((3,) if channels == 3 else ()), dtype=np.uint8)
        boxes = np.asarray([b for _, b in cases], np.float64)
        refs = [sr.preprocess(frames, boxes[i:i + B], S) for i in range(0, len(boxes), B)]
        ref = {k: np.concatenate([r[k] for r in refs]) for k in refs[0]}
        names = [n for n, _ in cases]
        side = ref["clip_bbox"][:, 2] - ref["clip_bbox"][:, 0]
        assert side[names.index("side_eq_S")] == S and side[names.index("larger")] > max(H, W)
        tl = boxes[names.index("corner_tl")]
        x1f = (tl[0] + tl[2]) / 2 - max(tl[2] - tl[0], tl[3] - tl[1]) * 1.2 / 2
        assert side[names.index("tiny")] < S and x1f < 0 and x1f != np.floor(x1f)
        assert ref["clip_bbox"][names.index("corner_tl"), 0] == np.ceil(x1f)     # truncation towards zero
        assert ref["status"].tolist() == [int(n == "empty") for n in names]
        _REF[key] = (frames, boxes, ref)
    return _REF[key]


def _assert_equal_outputs(o, ref, what):
    assert np.array_equal(o["status"].cpu().numpy(), ref["status"]), what
    assert np.array_equal(o["clip_bbox"].cpu().numpy(), ref["clip_bbox"].astype(np.float32)), what
    got = o["crops"].cpu().numpy()
    if not np.array_equal(got, ref["crops"]):
        d = np.abs(got.astype(np.int64) - ref["crops"].astype(np.int64))
        raise AssertionError(f"{what}: {int((d != 0).sum())} of {d.size} crop values differ, max {d.max()} LSB")
    assert np.array_equal(o["images"].cpu().numpy(), ref["images"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("channels,H,W,S,B", [(1, 160, 200, 32, 6), (3, 160, 200, 64, 4), (1, 1200, 1920, 416, 3),
                                              (1, 1200, 1920, 300, 2)])
def test_submission_hip_matches_restatement(gpu_device, channels, H, W, S, B):
    """Every box kind of _case_boxes, launched B at a time (the kinds outnumber the smaller
    batches, so a configuration takes more than one launch of its batch size)."""
    from spe.datasets import SpeedSubmissionTransform
    frames, boxes, ref = _reference(channels, H, W, S, B)
    dev_frames = torch.from_numpy(frames).to(gpu_device)
    t = SpeedSubmissionTransform(S)
    for i in range(0, len(boxes), B):
        o = t(dev_frames, boxes[i:i + B], crops=True)
        torch.cuda.synchronize()
        _assert_equal_outputs(o, {k: v[i:i + B] for k, v in ref.items()}, f"boxes {i}..{i + B - 1}")


@pytest.mark.gpu
def test_submission_hip_matches_reference_fixture(gpu_device, golden):
    from spe.datasets import SpeedSubmissionTransform
    g = golden
    S = int(g["size"])
    t = SpeedSubmissionTransform(S)
    big = g["frame_index"] < 0
    for sel in (np.nonzero(big)[0], np.nonzero(~big)[0]):
        frames = torch.from_numpy(np.stack([g["frames"][i] for i in sel])).to(gpu_device)
        o = t(frames, g["bbox"][sel], crops=True)
        torch.cuda.synchronize()
        assert (o["status"] == 0).all()
        assert np.array_equal(o["clip_bbox"].cpu().numpy(), g["clip_bbox"][sel].astype(np.float32))
        assert np.array_equal(o["crops"].cpu().numpy(), g["crops"][sel][..., 0])
        assert np.array_equal(o["images"].cpu().numpy(), g["images"][sel])


@pytest.mark.gpu
def test_submission_nullable_outputs(gpu_device):
    from spe import _lib
    from spe.datasets import SpeedSubmissionTransform
    frames, boxes, _ = _reference(1, 160, 200, 32, 6)
    boxes = boxes[:6]
    f = torch.from_numpy(frames).to(gpu_device)
    t = SpeedSubmissionTransform(32)
    both = t(f, boxes, crops=True)
    only_images = t(f, boxes)
    only_crops = t(f, boxes, crops=True, images=False)
    torch.cuda.synchronize()
    assert "crops" not in only_images and "images" not in only_crops
    assert torch.equal(only_images["images"], both["images"]) and torch.equal(only_crops["crops"], both["crops"])
    for o in (only_images, only_crops):
        assert torch.equal(o["clip_bbox"], both["clip_bbox"]) and torch.equal(o["status"], both["status"])
    bb = torch.from_numpy(boxes).to(gpu_device)
    rc = _lib.lib().spe_preprocess_submission(_lib.stream_ptr(), _lib.ptr(f), 6, 160, 200, 1, _lib.ptr(bb), 32, None,
                                              None, _lib.ptr(both["clip_bbox"]), _lib.ptr(both["status"]))
    assert rc == -1                                              # SPE_E_ARG
    # status itself is nullable
    clip = torch.empty_like(both["clip_bbox"])
    rc = _lib.lib().spe_preprocess_submission(_lib.stream_ptr(), _lib.ptr(f), 6, 160, 200, 1, _lib.ptr(bb), 32, None,
                                              _lib.ptr(only_crops["crops"]), _lib.ptr(clip), None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(clip, both["clip_bbox"])


@pytest.fixture(scope="module")
def small_model(gpu_device):
    """The smallest model configuration of tests/test_gpu_pipeline.py, label-diverse weights."""
    from spe.config import SpeConfig
    from spe.models import DETR
    from spe.synthetic import bench_weights
    cfg = SpeConfig(input_size=128, num_queries=11, enc_layers=2, dec_layers=2)

    def hs_fn(w, images):
        m = DETR(cfg, dtype="fp32")
        m.load_state_dict(w)
        return m(torch.from_numpy(images).to(gpu_device), return_hs=True)["hs"].cpu().numpy()

    w = bench_weights(cfg, 3, hs_fn)
    m = DETR(cfg, dtype="fp32")
    m.load_state_dict(w)
    m2 = DETR(cfg, dtype="fp32x3")       # the ensemble's second member: the same weights, split-bf16 compute
    m2.load_state_dict(w)
    return cfg, m, m2


def _e2e_inputs():
    rng = np.random.Generator(np.random.PCG64(23))
    H, W = 160, 200
    yy, xx = np.mgrid[0:H, 0:W]
    frames = [np.clip(np.rint(100 + 70 * np.sin(xx / (6.0 + i)) * np.cos(yy / 9.0) + rng.normal(0, 12, (H, W))), 0, 255)
              .astype(np.uint8) for i in range(5)]
    names = ["img5.jpg", "img1.jpg", "img4.jpg", "img2.jpg", "img3.jpg"]
    files = {n: _jpeg(f, quality=90, progressive=(i == 3)) for i, (n, f) in enumerate(zip(names, frames))}
    boxes = [[40.0, 30.0, 150.0, 120.0], [-8.5, 20.0, 90.0, 140.0], [120.0, 90.0, 230.0, 170.0],
             [60.2, 10.9, 170.4, 150.1], [230.0, 50.0, 250.0, 70.0]]          # the last: off-frame, status 1
    anns = {n: [b + [0.9], [0.0, 0.0, 10.0, 10.0, 0.1]] for n, b in zip(names, boxes)}
    return H, W, names, files, anns


@pytest.mark.gpu
def test_u8_entry_on_submission_crops_equals_fp32_entry(gpu_device, small_model):
    """spe_forward_stages_u8 on crops_u8 == spe_forward on images, bit for bit (include/spe.h)."""
    from spe.datasets import SpeedSubmissionTransform
    cfg, m, _ = small_model
    frames, boxes, _ = _reference(1, 160, 200, 32, 6)
    t = SpeedSubmissionTransform(cfg.input_size)(torch.from_numpy(frames[:2]).to(gpu_device), boxes[:2], crops=True)
    a = m(t["crops"], clip_bbox=t["clip_bbox"])
    b = m(t["images"], clip_bbox=t["clip_bbox"])
    torch.cuda.synchronize()
    assert t["crops"].dtype == torch.uint8 and t["images"].dtype == torch.float32
    for k in ("pred_logits", "pred_points", "points_px", "probs"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("ensemble", [False, True])
def test_generate_submission_end_to_end(gpu_device, small_model, ensemble):
    """From JPEG bytes (4 baseline gray files, 1 progressive that the device decoder refuses; batch
    size 2, so the progressive file shares a batch and the last batch is short) == the log assembled
    by hand from Pillow's decode, the restatement's crops and clip_bbox, the same model through its
    u8 entry and the solver's batched call."""
    import argparse
    from spe.datasets import JpegDecoder
    from spe.engine import generate_submission
    from spe.solver import Multi_Mean_PoseSolver, SimplePoseSolver
    cfg, m, m2 = small_model
    H, W, names, files, anns = _e2e_inputs()
    solver = Multi_Mean_PoseSolver(argparse.Namespace(repro=25)) if ensemble else SimplePoseSolver(argparse.Namespace(repro=20))
    models = [m, m2] if ensemble else m
    dec = JpegDecoder(H, W, max_bytes=max(map(len, files.values())))
    st = dec(*JpegDecoder.pack([files[n] for n in names], gpu_device))["status"].cpu().tolist()
    assert st == [0, 0, 0, 1, 0]                                 # the progressive file is refused on the device
    log = generate_submission(models, None, anns, files.__getitem__, solver, gpu_device, 2, cfg.input_size, decoder=dec)

    decoded = np.stack([np.asarray(Image.open(io.BytesIO(files[n]))) for n in names])
    ref = sr.preprocess(decoded, np.asarray([anns[n][0][:4] for n in names], np.float64), cfg.input_size)
    assert ref["status"].tolist() == [0, 0, 0, 0, 1]
    want = {}
    for i in range(0, 5, 2):
        crops = torch.from_numpy(ref["crops"][i:i + 2]).to(gpu_device)
        clip = torch.from_numpy(ref["clip_bbox"][i:i + 2].astype(np.float32)).to(gpu_device)
        o = m(crops, clip_bbox=clip)
        if ensemble:
            o2 = m2(crops, clip_bbox=clip)
            p = solver.solve_batch_multi([o["points_px"], o2["points_px"]], [o["probs"], o2["probs"]])
        else:
            p = solver.solve_batch(o["points_px"], o["probs"])
        quat, tvec, status = p["quat"].double().cpu().numpy(), p["tvec"].cpu().numpy(), p["status"].cpu().numpy()
        for j, n in enumerate(names[i:i + 2]):
            ok = status[j] in (0, 3) and ref["status"][i + j] == 0
            want[n] = {"quat_pr": np.around(quat[j] if ok else np.zeros(4), 6).tolist(),
                       "tvec_pr": np.around(tvec[j] if ok else np.zeros(3), 6).tolist()}
    print("solved poses:", sum(any(r["tvec_pr"]) for r in want.values()), "of", len(want))
    assert list(log) == names and log == want
    assert log[names[4]] == {"quat_pr": [0.0] * 4, "tvec_pr": [0.0] * 3}
