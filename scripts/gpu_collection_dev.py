#!/usr/bin/env python
"""A database of images whose descriptors are CUDA tensors: device adds and device results against the round trip they replace.

64 images x 10 000 rows x 128, once uint8 and once float16 (N(0, 1) values: the float32 route), and a 10 000-row query.

  add     host    for every image: tensor.cpu().numpy() (float16: .float() first), then Collection.add -- the only way into a
                  collection before fm_collection_add_dev
          device  for every image: Collection.add_from_device on the tensor's memory (torchmatch.Collection.add)
  knn2    host    Collection.knn(q, 2), then torch.from_numpy(...).cuda() of the three arrays
          device  Collection.knn_dev into three CUDA tensors

Each timed repetition starts and ends with a device synchronise (host clock around work that ends in a synchronise), the two
paths alternate, the first repetitions are warm-up, medians are reported with the spread.  The outputs of the two collections
are compared bit for bit first.  `python scripts/gpu_collection_dev.py` runs every step as a child of its own under `timeout`
and stops at the first that fails; `--step NAME` is one step.  Writes profiles/collection_dev.json (or --out)."""
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

N_IMAGES, ROWS, NQ = 64, 10000, 10000
STEPS = {"u8": 420, "f16": 420}          # step -> time limit of its child, seconds


def run_step(kind, reps, warmup):
    import numpy as np
    import torch
    import fastmatch_amd
    from fastmatch_amd import synth, torchmatch
    ctx = fastmatch_amd.Context(0)
    rng = np.random.default_rng(7)
    if kind == "u8":
        images = [torch.from_numpy(synth.synth_sift(ROWS, rng)).cuda() for _ in range(N_IMAGES)]
        qt = torch.from_numpy(synth.synth_sift(NQ, rng)).cuda()
    else:
        images = [torch.from_numpy(rng.standard_normal((ROWS, 128)).astype(np.float32)).to(torch.float16).cuda() for _ in range(N_IMAGES)]
        qt = torch.from_numpy(rng.standard_normal((NQ, 128)).astype(np.float32)).to(torch.float16).cuda()
    qb = torchmatch.bank(qt, float_route=kind != "u8", context=ctx)
    stream = torch.cuda.current_stream().cuda_stream
    host_c = ctx.collection()
    dev_c = torchmatch.Collection(context=ctx)

    def host_add():
        host_c.clear()
        for t in images:
            host_c.add((t if kind == "u8" else t.float()).cpu().numpy())

    def device_add():
        dev_c.clear()
        for t in images:
            dev_c.add(t)

    def host_knn():
        img, idx, dist = host_c.knn(qb, 2)
        return torch.from_numpy(img).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(dist).cuda()

    def device_knn():
        img = torch.empty((NQ, 2), dtype=torch.int32, device="cuda")
        idx = torch.empty((NQ, 2), dtype=torch.int32, device="cuda")
        dist = torch.empty((NQ, 2), dtype=torch.float32, device="cuda")
        dev_c._coll.knn_dev(qb, 2, img.data_ptr(), idx.data_ptr(), dist.data_ptr(), consumer_stream=stream)
        return img, idx, dist

    host_add(); device_add()
    a, b = host_knn(), device_knn()
    torch.cuda.synchronize()
    same = bool(host_c.info() == dev_c.info() and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)))
    res = {"step": kind, "n_images": N_IMAGES, "rows_per_image": ROWS, "nq": NQ, "reps": reps, "warmup": warmup,
           "outputs_identical": same, "collection": list(dev_c.info()), "device": ctx.device_name()}
    for what, pair in (("add", (("host", host_add), ("device", device_add))), ("knn2", (("host", host_knn), ("device", device_knn)))):
        times = {"host": [], "device": []}
        for r in range(warmup + reps):
            for label, f in pair:                                  # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                if r >= warmup:
                    times[label].append((time.perf_counter() - t0) * 1e3)
        for label, v in times.items():
            v = sorted(v)
            res["%s_%s_ms" % (what, label)] = {"median": statistics.median(v), "min": v[0], "max": v[-1],
                                               "p10": v[len(v) // 10], "p90": v[(len(v) * 9) // 10]}
        res[what + "_speedup_median"] = res[what + "_host_ms"]["median"] / res[what + "_device_ms"]["median"]
    res["add_device_ms_per_image"] = res["add_device_ms"]["median"] / N_IMAGES
    res["add_host_ms_per_image"] = res["add_host_ms"]["median"] / N_IMAGES
    dev_c.close(); host_c.close(); qb.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collection_dev.json"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run_step(args.step, args.reps, args.warmup)))
        return 0
    results = []
    for name in ("u8", "f16"):
        r = subprocess.run(["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.abspath(__file__), "--step", name,
                            "--reps", str(args.reps), "--warmup", str(args.warmup)], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.stderr.write("step %s ended with status %d: stopping\n" % (name, r.returncode))
            return 1
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"results": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
