"""Every entry point that ends in the cross-check tail (election, decode, ordered compaction, delivery), once, at the
shape of tests/test_xcheck_delivery_gpu.py: 700 x 900 rows, two splits; a planted integer pair, a pair in the float32-root
tie range, a non-integer float32 pair, a binary pair.  For a kernel trace (the table of kernel name against calls must not
change when the host code behind these calls is rearranged):
  rocprofv3 --kernel-trace --stats -d DIR -o tail --output-format csv -- python scripts/gpu_tail_launches.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fastmatch_amd as fm
from fastmatch_amd import synth
import kat

NQ, NT, CAP = 700, 900, 50
ctx = fm.Context(0)
ctx.set_option("nsplit", 2)
rng = np.random.default_rng(3)
Q, T, _ = synth.planted_pair(NQ, NT, seed=NQ + NT)
FQ, FT = kat.far_banks(NQ, NT, np.random.default_rng(5))
jit = lambda a: a.astype(np.float32) + rng.uniform(-0.5, 0.5, a.shape).astype(np.float32)
BQ, BT = rng.integers(0, 256, (NQ, 32), dtype=np.uint8), rng.integers(0, 256, (NT, 32), dtype=np.uint8)
pairs = {"planted": (ctx.bank(Q), ctx.bank(T)), "far": (ctx.bank(FQ), ctx.bank(FT)), "f32": (ctx.bank(jit(Q)), ctx.bank(jit(T)))}
for qb, _ in pairs.values():
    qb.set_selfdist(ctx.self_dist(qb))
bq, bt = ctx.bank_binary(BQ), ctx.bank_binary(BT)
dev = torch.device("cuda", 0)
pin = lambda n: tuple(ctx.pinned_empty(n, dt) for dt in (np.int32, np.int32, np.float32, np.float64))
rows, cnt = torch.zeros((3, NQ, 3), dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
d_t, d_d = torch.zeros(NQ, dtype=torch.int32, device=dev), torch.zeros(NQ, dtype=torch.float32, device=dev)
d_k = torch.zeros(NQ, dtype=torch.int64, device=dev)
hc = ctx.pinned_empty(3, np.int64)
torch.cuda.synchronize()
for name, (qb, tb) in pairs.items():
    tau = 2551.0 if name == "far" else 0.7
    ctx.xcheck1(qb, tb)
    ctx.xcheck1_dev(qb, tb, d_t.data_ptr(), d_d.data_ptr())
    ctx.xcheck1_keys(qb, tb)
    ctx.xcheck1_keys_dev(qb, tb, 0, d_k.data_ptr())
    ctx.match_ratio(qb, tb, tau)
    ctx.match_accepted(qb, tb, tau)                                   # staged
    ctx.match_accepted(qb, tb, tau, out=pin(CAP))                     # direct
    ctx.match_accepted(qb, tb, tau, out=pin(NQ + CAP))                # staged despite page-locked arrays
    ctx.match_accepted_dev(qb, tb, tau, rows.data_ptr(), cnt.data_ptr(), CAP)
    ctx.knn2_ratio(qb, tb, 0.8)
    ctx.knn2_ratio_dev(qb, tb, 0.8, rows.data_ptr(), cnt.data_ptr(), CAP, want_count=True)
    if name != "f32":
        ctx.match_accepted_async(qb, tb, tau, pin(CAP), ctx.pinned_empty(1, np.int64))
        ctx.match_accepted_dev_async(qb, tb, tau, rows.data_ptr(), cnt.data_ptr(), CAP, h_count=hc[:1])
        ctx.match_accepted_batch([(qb, tb)], tau, [pin(CAP)], [ctx.pinned_empty(1, np.int64)])
    ctx.sync()
ctx.xcheck1(bq, bt)
ctx.xcheck1_dev(bq, bt, d_t.data_ptr(), d_d.data_ptr())
ctx.knn2_ratio(bq, bt, 0.8)
three = [pairs["planted"], pairs["f32"], pairs["far"]]
ctx.match_accepted_batch(three, 0.7, [pin(CAP) for _ in three], [ctx.pinned_empty(1, np.int64) for _ in three])
ctx.match_accepted_dev_batch(three, 0.7, rows.data_ptr(), cnt.data_ptr(), NQ, h_counts=hc)
two = [pairs["planted"], pairs["far"], pairs["planted"]]
ctx.match_accepted_batch(two, 0.7, [pin(CAP) for _ in two], [ctx.pinned_empty(1, np.int64) for _ in two])
ctx.match_accepted_dev_batch(two, 0.7, rows.data_ptr(), cnt.data_ptr(), NQ, h_counts=hc)
ctx.sync()
torch.cuda.synchronize()
print("tail launches done")
