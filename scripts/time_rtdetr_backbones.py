"""bf16 forward of the RT-DETR model at B = 64 behind GhostNetV2, MobileNetV3_Large and PResNet-vd r18: ms per step (HIP
events, median of 5 x 20 steps after 10 warm-up steps) and the per-kind launch table of the built-in profiler
(spe_model_profile_*).  Run from the repository root; writes bench_out/time_rtdetr_backbones.json
(profiles/r7_rtdetr_mbv3l_vs_r18_b64.json and profiles/r8_rtdetr_backbones_b64.json are such runs; the latter has
all three backbones and, per backbone, backbone_ms / backbone_share: the launch kinds up to the hybrid encoder)."""
import ctypes, json, os, sys
sys.path[:0] = ["satellite-pose-estimation_amd", "oracle", "tests"]
import numpy as np, torch
from spe import _lib
from spe.rtdetr import RTDETR
from spe.rtdetr_spec import RtdetrConfig, random_rtdetr_weights

dev = torch.device("cuda:0")
B = 64
out = {}
# launch kinds of the backbone stage (r18: rt.conv.1x1 / rt.conv.3x3 are shared with the hybrid encoder's CSP
# layers, so its figure is an upper bound)
BACKBONE_KINDS = {"ghostv2": ("conv.stem.gh", "conv.pw.mb", "conv.dw", "rt.se", "conv.ghost", "conv.dfc", "eltwise.pool2"),
                  "mbv3l": ("conv.stem.mb", "conv.pw.mb", "conv.dw", "rt.se"),
                  "r18": ("eltwise.pack", "rt.conv.stem", "eltwise.maxpool", "rt.conv.short", "rt.conv.1x1", "rt.conv.3x3")}
for name, cfg in (("ghostv2", RtdetrConfig(backbone="ghostnetv2")), ("mbv3l", RtdetrConfig(backbone="mobilenetv3_large")),
                  ("r18", RtdetrConfig(depth=18))):
    m = RTDETR(cfg, "bf16", aux_outputs=False)
    m.load_state_dict(random_rtdetr_weights(cfg, 1))
    x = torch.randn(B, 3, 256, 256, device=dev)
    for _ in range(10):
        m(x)
    torch.cuda.synchronize()
    ms = []
    for rep in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            m(x)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 20)
    L = _lib.lib()
    L.spe_model_profile_begin(m._h, b"")
    for _ in range(5):
        m(x)
    torch.cuda.synchronize()
    n = L.spe_model_profile_end(m._h)
    kinds = {}
    for i in range(n):
        kb = ctypes.create_string_buffer(64)
        t, f, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        L.spe_model_profile_get(m._h, i, kb, 64, ctypes.byref(t), ctypes.byref(f), ctypes.byref(by))
        k = kinds.setdefault(kb.value.decode(), [0, 0.0, 0.0, 0.0])
        k[0] += 1; k[1] += t.value / 5; k[2] += f.value / 5; k[3] += by.value / 5
    out[name] = {"ms_per_step_median": float(np.median(ms)), "ms_all": ms, "img_per_s": B / float(np.median(ms)) * 1e3,
                 "kinds": {k: {"launches": v[0] // 5, "ms": v[1], "gflops": v[2] / 1e9, "mbytes": v[3] / 1e6,
                               "gb_per_s": v[3] / max(v[1], 1e-9) / 1e6} for k, v in sorted(kinds.items())}}
    bb = sum(v["ms"] for k, v in out[name]["kinds"].items() if k in BACKBONE_KINDS[name])
    out[name]["backbone_ms"] = bb
    out[name]["backbone_share"] = bb / max(sum(v["ms"] for v in out[name]["kinds"].values()), 1e-9)
os.makedirs("bench_out", exist_ok=True)
json.dump(out, open("bench_out/time_rtdetr_backbones.json", "w"), indent=1)
for n, r in out.items():
    print(n, "ms/step", r["ms_per_step_median"], "img/s", r["img_per_s"], "backbone ms", r["backbone_ms"], "share", r["backbone_share"])
    for k, v in r["kinds"].items():
        print("   %-18s n=%3d  %8.3f ms  %8.1f GB/s" % (k, v["launches"], v["ms"], v["gb_per_s"]))
