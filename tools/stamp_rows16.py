"""Diagnostic: per-phase s_memtime stamps of the row-split step kernel
(ppo_rows16.h) at the headline shape.  Run with
MADRONA_LEARN_LIB=madrona-learn_amd/variants/libmlearn_stamps.so
(tools/build_stamps.sh)."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "madrona-learn_amd")]
import bench  # noqa: E402
from madrona_learn import _native as nat  # noqa: E402

dev = torch.device("cuda:0")
mgr = bench.make(dev, 65536, 0, 65536, use_graph=False)
mgr.update_iter()
torch.cuda.synchronize()
L = nat.lib()
L.mlearn_debug_set_stamp_buffer.argtypes = [ctypes.c_void_p]
algo = mgr.algo
ps, ts = mgr.state.policy_states, mgr.state.train_states
M = algo.mb * algo.bptt
tiles = ((M + 63) // 64 * 64) // 16  # 16-row tiles
buf = torch.zeros((tiles, 16), dtype=torch.int64, device=dev)
L.mlearn_debug_set_stamp_buffer(buf.data_ptr())
names = {1: "L0 x loads + fwd + stats", 2: "X0/dZ0 stores + LN0 apply",
         3: "task loads + L1 product + stats", 4: "A0 store + LN1 apply",
         5: "heads + A1 store + logits", 6: "loss", 7: "dhead store + hb sums",
         8: "head bwd + LN1 bwd", 9: "W1^T product", 10: "dZ1 store",
         11: "Z0 recompute", 12: "LN0 bwd"}
for it in range(3):
    buf.zero_()
    seqs = algo.perm[0, :algo.mb]
    nat.check(L.mlearn_ppo_minibatch_grad(ps.desc, algo.view, nat.ptr(seqs), algo.mb,
                                          nat.ptr(algo.adv_stats[0, 0]), algo.hp,
                                          nat.ptr(ts.grads), None, nat.ptr(algo.ws),
                                          nat.stream_handle()))
    torch.cuda.synchronize()
st = buf.cpu().numpy().astype(np.int64)
w0 = st[0::2]  # tile 0 rows of each wave: [13] entry, [14] after prologue, [15] end
print("per wave (cycles, median / max): prologue", np.median(w0[:, 14] - w0[:, 13]),
      (w0[:, 14] - w0[:, 13]).max(), "| tiles", np.median(st[1::2, 12] - w0[:, 0]),
      "| epilogue (last stores done)", np.median(w0[:, 15] - st[1::2, 12]),
      (w0[:, 15] - st[1::2, 12]).max(), "| entry..end", np.median(w0[:, 15] - w0[:, 13]),
      (w0[:, 15] - w0[:, 13]).max())
# the head of the launch: kernel entry to the end of tile 0's first layer
# (staging, barrier, the wave's mb_seq entry, the gather, 32 MFMAs), and the
# same phase of the last tile, which has no prologue in front of it
h0 = w0[:, 1] - w0[:, 13]
l0n = st[1::2, 1] - st[1::2, 0]
print("tile 0 kernel entry -> end of layer 0 (median / mean / max):", np.median(h0),
      float(h0.mean()), h0.max(), "| of which after the prologue", np.median(w0[:, 1] - w0[:, 14]),
      "| last tile's layer 0", np.median(l0n), float(l0n.mean()), l0n.max())
# split staging (tile 1's row, slots 13 / 14: the wave's arrival at the
# workgroup barrier and the point where its prologue loads were all issued --
# with -DML_STAMPS_LANDING, on the staging waves, where the images had landed;
# zero in builds from before the split), per wave group, from the wave's entry
if st[1::2, 13].any():
    ent = w0[:, 13]
    cols = {"prologue loads issued": st[1::2, 14] - ent, "arrival at the barrier": st[1::2, 13] - ent,
            "barrier release": w0[:, 14] - ent, "end of layer 0": h0,
            "waiting at the barrier": w0[:, 14] - st[1::2, 13]}
    for gname, sl in (("waves 0-3", slice(0, 4)), ("waves 4-7", slice(4, 8))):
        print(f"{gname} (cycles from the wave's entry, median / max):",
              " | ".join(f"{k} {np.median(v.reshape(-1, 8)[:, sl]):.0f} {v.reshape(-1, 8)[:, sl].max()}"
                         for k, v in cols.items()))
    print("by wave index (median): arrival", [int(x) for x in np.median(cols["arrival at the barrier"].reshape(-1, 8), 0)],
          "release", [int(x) for x in np.median(cols["barrier release"].reshape(-1, 8), 0)])
# per workgroup (8 waves, one CU): wave time entry..end by wave index, and the
# spread inside a workgroup vs across workgroups
tw = (w0[:, 15] - w0[:, 13]).reshape(-1, 8)
print("wave time by wave index (median over WGs):", [int(x) for x in np.median(tw, 0)])
print("WG max/min ratio median", float(np.median(tw.max(1) / tw.min(1))),
      "| WG max: median", float(np.median(tw.max(1))), "max", int(tw.max()),
      "| WG mean: min", float(tw.mean(1).min()), "max", float(tw.mean(1).max()))
end_rel = (w0[:, 15] - w0[:, 13].reshape(-1, 8).min(1).repeat(8)).reshape(-1, 8)
print("WG finish (from its first wave's entry): median", float(np.median(end_rel.max(1))),
      "max", int(end_rel.max()))
ok = st[:, 12] != 0
st = st[ok]
print("tiles stamped", int(ok.sum()), "of", tiles, "- cycles per phase (median / mean / max):")
for i in range(1, 13):
    d = st[:, i] - st[:, i - 1]
    print(f"  {names[i]:34s} {np.median(d):9.0f} {d.mean():9.0f} {d.max():9.0f}")
tot = st[:, 12] - st[:, 0]
print("tile total median", np.median(tot), "mean", tot.mean())
print("kernel span", st[:, 12].max() - st[:, 0].min())
first = st[:, 0] - st[:, 0].min()
print("tile start spread: median", np.median(first), "max", first.max())
