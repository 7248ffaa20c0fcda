"""Per-block timeline + phase cycles of the bench frame's blend kernels.  Needs the
-DPR_BLEND_PROFILE variant:
    python -m pertrenderer_amd.build_native --out pertrenderer_amd/libpertrender_prof.so -D PR_BLEND_PROFILE
    PR_NATIVE_LIB=pertrenderer_amd/libpertrender_prof.so python tools/blend_prof.py
Forward phases: setup / slots / MC rast / pixel / MC argmax / output.  Backward: setup / B1 / B2 /
B5 / B6 / B7 / B8 / reduction.  Phases are summed over a block's passes.
--split: the variant was also built with -D PR_BLEND_PROF_SPLIT_B2 -D PR_BLEND_PROF_SPLIT_1A: the
forward's "slots" is then 1a's records and queue appends and "1a_load" its load round(s), the
backward's "B2" its colour gathers and "B2pix+red" its per-pixel part plus the final reduction.

Only blocks that run the phases are recorded (the empty-block shortcut returns before the record).
Per kernel it also prints how the blocks landed on the chip: entries (valid slots + 1 per pixel of
the block) and busy time (sum of the blocks' durations) per XCD and per CU, the non-empty blocks
of the first generation, the start of the last heavy block and the span.  PR_BLEND_ORDER selects
the block order under test (0: linear, 1: centre-out forward, 12: rotated, ...)."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from pertrenderer_amd import _native as nat  # noqa: E402

import argparse  # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("--config", choices=sorted(bench.CONFIGS), default="cfg2")
ap.add_argument("--dense", action="store_true", help="the dense-fragment microbench (bench.dense_roofline's blend)")
ap.add_argument("--split", action="store_true", help="name the split stamps (see above)")
ap.add_argument("--save", help="also write the raw records (2 x 65536 x 12 int64) to this .npy")
args = ap.parse_args()
cfg = bench.CONFIGS[args.config]
# blocks past the first 65536 are not recorded (a cfg4 frame has 524288: images 0-1 only)
if args.dense:
    bench.dense_roofline(torch.device("cuda:0"), cfg["image_size"], cfg["K"], cfg["samples"], iters=2,
                         Sr=cfg.get("rast_samples"))
else:
    wl = bench.Workload(torch.device("cuda:0"), cfg["image_size"], cfg["K"], cfg["samples"], batch=cfg["batch"])
    for _ in range(3):
        wl.forward().backward()
        torch.cuda.synchronize()
lib = nat.load()
NB = 1 << 16
REC = 12
buf = np.zeros(2 * NB * REC, dtype=np.int64)
assert lib.pr_blend_prof_dump(ctypes.c_void_p(buf.ctypes.data), ctypes.c_size_t(buf.nbytes)) == 0
rec = buf.reshape(2, NB, REC)
if args.save:
    np.save(args.save, rec[:, :(rec[:, :, REC - 1] & 1).nonzero()[1].max() + 1])
print(f"config {args.config}{' dense' if args.dense else ''}  PR_BLEND_ORDER={os.environ.get('PR_BLEND_ORDER', '(default)')}")


def spread(name, v, unit=""):
    v = np.asarray(v, dtype=np.float64)
    m = v.mean()
    print(f"  {name}: min {v.min():.0f} mean {m:.0f} max {v.max():.0f}{unit}  (max/mean {v.max() / m:.2f}, "
          f"min/mean {v.min() / m:.2f}, n {len(v)})")


FWD = ["setup", "slots", "rast", "pixel", "argmax", "out"] + (["1a_load"] if args.split else [])
BWD = ["setup", "B1", "B2", "B5", "B6", "B7", "B8", "B2pix+red" if args.split else "red"]
for w, name, ph in ((0, "blend_fwd", FWD), (1, "blend_bwd", BWD)):
    r = rec[w][(rec[w][:, REC - 1] & 1) == 1]
    t0 = r[:, 0].min()
    st, en = (r[:, 0] - t0) / 100.0, (r[:, 1] - t0) / 100.0
    print(f"{name}: blocks {len(r)} span {en.max():.1f} us, last start {st.max():.1f}, dur mean {(en - st).mean():.1f} "
          f"max {(en - st).max():.1f}")
    pm = (r[:, 2:2 + len(ph)].mean(0) / 2400).round(2)
    px = (r[:, 2:2 + len(ph)].max(0) / 2400).round(2)
    print("  phase us mean", dict(zip(ph, pm.tolist())), "\n  phase us max ", dict(zip(ph, px.tolist())))
    hist = np.histogram(st, bins=8)[0]
    print("  start histogram", hist.tolist())
    dur = en - st
    for q in (50, 90, 99):
        print(f"  duration p{q} {np.percentile(dur, q):.1f} us")
    for i in np.argsort(-dur)[:5]:  # the longest blocks: start, duration, phases
        print(f"  long block start {st[i]:.1f} dur {dur[i]:.1f} phases",
              dict(zip(ph, (r[i, 2:2 + len(ph)] / 2400).round(2).tolist())))
    hv = ((r[:, REC - 1] >> 8) & 0xffffff) >= 0.8 * ((r[:, REC - 1] >> 8) & 0xffffff).max()
    print("  heavy blocks' phase us mean", dict(zip(ph, (r[hv, 2:2 + len(ph)].mean(0) / 2400).round(2).tolist())),
          "\n  heavy blocks' phase us max ", dict(zip(ph, (r[hv, 2:2 + len(ph)].max(0) / 2400).round(2).tolist())))
    # where the blocks ran: XCC_ID in bits 32-35 of the hw word, SE / SH / CU of HW_ID below
    ent = (r[:, REC - 1] >> 8) & 0xffffff
    disp = r[:, REC - 1] >> 32
    xcd = (r[:, 10] >> 32) & 0xf
    cu = r[:, 10] & 0xf00007f00
    xs, cs = np.unique(xcd), np.unique(cu)
    print(f"  placement: {len(xs)} XCDs, {len(cs)} CUs seen; dispatch index % 8 == XCD for "
          f"{(disp % 8 == xcd).mean() * 100:.1f} % of the blocks (other fixed mapping: "
          f"{max(np.bincount(((xcd - disp) % 8).astype(np.int64), minlength=8)) / len(r) * 100:.1f} %)")
    spread("entries per XCD", [ent[xcd == x].sum() for x in xs])
    spread("busy us per XCD", [dur[xcd == x].sum() for x in xs])
    spread("entries per CU", [ent[cu == c].sum() for c in cs])
    spread("busy us per CU", [dur[cu == c].sum() for c in cs])
    spread("blocks per CU", [(cu == c).sum() for c in cs])
    first_end = en.min()
    heavy = ent >= 0.8 * ent.max()
    print(f"  first generation (started before the first recorded block ended, {first_end:.1f} us): "
          f"{(st < first_end).sum()} of {len(r)} non-empty blocks; within 2 us: {(st < 2.0).sum()}")
    print(f"  heavy blocks (>= {int(0.8 * ent.max())} entries): {heavy.sum()}, last start {st[heavy].max():.1f} us, "
          f"last end {en[heavy].max():.1f} us; span {en.max():.1f} us")
    for x in xs:
        m = xcd == x
        print(f"    XCD {x}: blocks {m.sum():4d} entries {ent[m].sum():7d} busy {dur[m].sum():7.0f} us "
              f"last end {en[m].max():5.1f} us")
