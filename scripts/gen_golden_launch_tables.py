"""Records tests/golden/launch_tables.json: for every case of tests/helpers.py launch_table_cases(),
the launches one forward call makes, in issue order, as [kind, flops, bytes] (the per-launch profiler's
records).  tests/test_gpu_launch_table.py asserts a forward still makes exactly these launches.

    python scripts/gen_golden_launch_tables.py [--out FILE]

Run it on the commit whose launch sequence is the reference (before a change that must not alter it).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "satellite-pose-estimation_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "launch_tables.json"))
    args = ap.parse_args()
    import torch

    import helpers
    dev = torch.device("cuda:0")
    tables = {name: helpers.run_launch_table_case(name, dev) for name in helpers.launch_table_cases()}
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in tables.items()) + "\n}\n")
    print(f"{len(tables)} cases, {sum(len(v) for v in tables.values())} launches -> {args.out}")


if __name__ == "__main__":
    main()
