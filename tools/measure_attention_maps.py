"""Cost of the attention-map export on the MI355X: DETR.forward_with_attention against DETR.forward on the
same tree at BASELINE config 2's shape (416 x 416, 11 queries, 6 / 6 layers) with B = 8, and the map
kernel's own time and achieved write bandwidth from the per-launch profiler (kind "attn.map").

    python tools/measure_attention_maps.py [--out profiles/attention_maps_bench.json]

A diagnostic path: the numbers are reported, nothing is gated on them.
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "satellite-pose-estimation_amd"))

import torch  # noqa: E402

from spe import _lib  # noqa: E402
from spe.config import SpeConfig  # noqa: E402
from spe.models import DETR  # noqa: E402
from spe.synthetic import random_weights, synthetic_batch  # noqa: E402


def time_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def map_launches(m, fn):
    """(ms, bytes written) of every attn.map launch `fn` makes, from the per-launch profiler."""
    L = _lib.lib()
    _lib.check(L.spe_model_profile_begin(m._h, b"attn.map"), "spe_model_profile_begin")
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        n = L.spe_model_profile_end(m._h)
    kb = ctypes.create_string_buffer(64)
    ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    rows = []
    for i in range(n):
        _lib.check(L.spe_model_profile_get(m._h, i, kb, 64, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)),
                   "spe_model_profile_get")
        rows.append(ms.value)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attention_maps_bench.json"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=11)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = SpeConfig()                                   # config 2: 416 / 11 queries / 6 + 6 layers
    B, T, Q = args.batch, cfg.tokens, cfg.num_queries
    w = random_weights(cfg, 0)
    img = torch.from_numpy(synthetic_batch(cfg, B, 1)["images"]).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "input_size": cfg.input_size, "batch": B, "tokens": T, "queries": Q,
           "enc_map_bytes": B * T * T * 4, "dec_map_bytes": B * Q * T * 4, "warmup": args.warmup, "iters": args.iters,
           "modes": {}}
    for dtype in ("bf16", "fp32"):
        m = DETR(cfg, dtype=dtype)
        m.load_state_dict(w)
        maps = {"enc": torch.empty(B, T, T, device=dev), "dec": torch.empty(B, Q, T, device=dev)}
        fwd = time_ms(lambda: m(img), args.warmup, args.iters)
        att = time_ms(lambda: m.forward_with_attention(img, maps=maps), args.warmup, args.iters)
        enc_only = time_ms(lambda: m.forward_with_attention(img, maps={"enc": maps["enc"], "dec": None}), args.warmup,
                           args.iters)
        k = [map_launches(m, lambda: m.forward_with_attention(img, maps=maps)) for _ in range(3)][-1]
        r = {"forward_ms": fwd[0], "forward_with_attention_ms": att[0], "forward_with_enc_map_only_ms": enc_only[0],
             "forward_ms_min_max": fwd[1:], "forward_with_attention_ms_min_max": att[1:],
             "enc_map_kernel_ms": k[0], "dec_map_kernel_ms": k[1],
             "enc_map_write_GBps": res["enc_map_bytes"] / (k[0] * 1e-3) / 1e9,
             "dec_map_write_GBps": res["dec_map_bytes"] / (k[1] * 1e-3) / 1e9}
        res["modes"][dtype] = r
        print(dtype, json.dumps(r))
        del m
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
