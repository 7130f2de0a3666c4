"""Cost of the RT-DETR attention-map export on the MI355X: RTDETR.forward_with_attention against RTDETR.forward on
the same tree (r18, 256 x 256, B = 64, bf16 by default), and the two map launches' own times from the per-launch
profiler (kinds "rt.attn_map.aifi" and "rt.attn_map.deform").

    python tools/measure_rtdetr_attention.py [--out profiles/rtdetr_attention_bench.json]

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
from spe.rtdetr import RTDETR  # noqa: E402
from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights  # noqa: E402


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
    """{kind: ms} of the rt.attn_map.* launches `fn` makes, from the per-launch profiler."""
    L = _lib.lib()
    _lib.check(L.spe_model_profile_begin(m._h, b""), "spe_model_profile_begin")
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        n = L.spe_model_profile_end(m._h)
    kb = ctypes.create_string_buffer(64)
    ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    rows = {}
    for i in range(n):
        _lib.check(L.spe_model_profile_get(m._h, i, kb, 64, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)),
                   "spe_model_profile_get")
        if kb.value.startswith(b"rt.attn_map"):
            rows[kb.value.decode()] = ms.value
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rtdetr_attention_bench.json"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=11)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = RtdetrConfig(depth=18, input_size=256)
    B, Q = args.batch, cfg.num_queries
    L, T5 = sum(s * s for s in cfg.level_sizes), cfg.level_sizes[-1] ** 2
    m = RTDETR(cfg, dtype=args.dtype)
    m.load_state_dict(random_rtdetr_weights(cfg, 0))
    img = torch.randn(B, 3, 256, 256, generator=torch.Generator().manual_seed(1)).to(dev)
    fwd = time_ms(lambda: m(img), args.warmup, args.iters)
    att = time_ms(lambda: m.forward_with_attention(img), args.warmup, args.iters)
    k = [map_launches(m, lambda: m.forward_with_attention(img)) for _ in range(3)][-1]
    dec_bytes, enc_bytes = B * Q * (L + 96 * 3) * 4, B * T5 * T5 * 4
    res = {"device": torch.cuda.get_device_name(0), "depth": 18, "input_size": 256, "batch": B, "dtype": args.dtype,
           "queries": Q, "tokens": L, "aifi_tokens": T5, "dec_map_bytes": dec_bytes, "enc_map_bytes": enc_bytes,
           "warmup": args.warmup, "iters": args.iters, "forward_ms": fwd[0], "forward_ms_min_max": fwd[1:],
           "forward_with_attention_ms": att[0], "forward_with_attention_ms_min_max": att[1:], "kernel_ms": k,
           "deform_map_write_GBps": dec_bytes / (k["rt.attn_map.deform"] * 1e-3) / 1e9,
           "aifi_map_write_GBps": enc_bytes / (k["rt.attn_map.aifi"] * 1e-3) / 1e9}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
