#!/usr/bin/env python
"""Descriptors are CUDA tensors, results are wanted as CUDA tensors: the host-array path against the device path.

For a 100k x 100k uint8 pair and a 10k x 1M float32 pair, the time from "the descriptors are CUDA tensors" to "the 2-NN
lists are CUDA tensors", two ways in one process on one build:

  host    tensor -> numpy (device-to-host) -> Context.bank (host-to-device + preparation) -> Context.knn2 (sweep,
          device-to-host) -> torch.from_numpy(...).cuda() (host-to-device)
  device  torchmatch.bank (preparation kernels read the tensor in place) -> Context.knn_dev (the merge kernel writes the
          result tensors)

Each timed repetition starts and ends with a device synchronise (host clock around work that ends in a synchronise), the two
paths alternate, outputs of both are compared bit for bit first.  `python scripts/gpu_device_io.py` runs every shape as a
child of its own under `timeout` and stops at the first that fails; `--step NAME` is one shape.  Writes
profiles/device_io.json (or --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = {"u8_100k_x_100k": ("u8", 100000, 100000, 600), "f32_10k_x_1m": ("f32", 10000, 1000000, 900)}


def run_step(name, reps, warmup):
    import numpy as np
    import torch
    import fastmatch_amd
    from fastmatch_amd import synth, torchmatch
    kind, nq, nt, _ = STEPS[name]
    ctx = fastmatch_amd.Context(0)
    rng = np.random.default_rng(7)
    Q, T = synth.synth_sift(nq, rng), synth.synth_sift(nt, rng)
    if kind == "f32":
        Q = Q.astype(np.float32) + rng.uniform(-0.5, 0.5, Q.shape).astype(np.float32)
        T = T.astype(np.float32) + rng.uniform(-0.5, 0.5, T.shape).astype(np.float32)
    qt, tt = torch.from_numpy(Q).cuda(), torch.from_numpy(T).cuda()
    del Q, T
    stream = torch.cuda.current_stream().cuda_stream

    def host_path():
        qb, tb = ctx.bank(qt.cpu().numpy()), ctx.bank(tt.cpu().numpy())
        idx, dist = ctx.knn2(qb, tb)
        out = torch.from_numpy(idx).cuda(), torch.from_numpy(dist).cuda()
        qb.close(); tb.close()
        return out

    def device_path():
        qb, tb = torchmatch.bank(qt, context=ctx), torchmatch.bank(tt, context=ctx)
        idx = torch.empty((nq, 2), dtype=torch.int32, device="cuda")
        dist = torch.empty((nq, 2), dtype=torch.float32, device="cuda")
        ctx.knn_dev(qb, tb, 2, idx.data_ptr(), dist.data_ptr(), consumer_stream=stream)
        qb.close(); tb.close()
        return idx, dist

    a, b = host_path(), device_path()
    torch.cuda.synchronize()
    same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
    times = {"host": [], "device": []}
    for r in range(warmup + reps):
        for label, f in (("host", host_path), ("device", device_path)):        # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if r >= warmup:
                times[label].append((time.perf_counter() - t0) * 1e3)
    res = {"step": name, "kind": kind, "nq": nq, "nt": nt, "reps": reps, "warmup": warmup, "outputs_identical": same,
           "device": ctx.device_name()}
    for label, v in times.items():
        v = sorted(v)
        res[label + "_ms"] = {"median": statistics.median(v), "min": v[0], "max": v[-1],
                              "p10": v[len(v) // 10], "p90": v[(len(v) * 9) // 10]}
    res["speedup_median"] = res["host_ms"]["median"] / res["device_ms"]["median"]
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_io.json"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("at least 20 timed repetitions")
    if a.step:
        print(json.dumps(run_step(a.step, a.reps, a.warmup)))
        return 0
    results = []
    for name in STEPS:
        cmd = ["timeout", "-k", "10", str(STEPS[name][3]), sys.executable, os.path.abspath(__file__), "--step", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            print("step %s ended with status %d: stopping" % (name, p.returncode), file=sys.stderr)
            return 1
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"what": "CUDA tensors in -> 2-NN lists as CUDA tensors out, ms per pair end to end; host = tensor -> numpy -> "
                           "Context.bank -> knn2 -> numpy -> tensor, device = torchmatch.bank -> knn_dev", "results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
