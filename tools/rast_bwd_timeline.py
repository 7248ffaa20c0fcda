"""Per-tile timeline + phase times of rast_bwd_kernel on a bench frame.  Needs the -DPR_RAST_PROFILE variant:
    python -m pertrenderer_amd.build_native --out pertrenderer_amd/libpertrender_prof.so -D PR_RAST_PROFILE
    PR_NATIVE_LIB=pertrenderer_amd/libpertrender_prof.so python tools/rast_bwd_timeline.py collect OUT.npy
    python tools/rast_bwd_timeline.py OUT.npy [...]          (summary; no GPU)
Records (int64 x16 per tile): x y z slots t0 t1 hw_id setup scan grad transpose flush rounds faces
(d zbuf | d dists << 32 non-zero slots) (d bary non-zero | all-zero slots << 32); t0 / t1 in 100 MHz ticks,
the phases in s_memtime ticks (reported as their share of t1 - t0)."""
import os
import sys

import numpy as np

HEAVY = 700  # valid slots of a "heavy" tile (a full 8x2 tile at K = 50 has 800)


def collect(out):
    import ctypes

    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    from pertrenderer_amd import _native as nat
    name = os.environ.get("PR_PROF_CONFIG", "cfg2")
    cfg = bench.CONFIGS[name]
    wl = bench.Workload(torch.device("cuda:0"), cfg["image_size"], cfg["K"], cfg["samples"], batch=cfg["batch"],
                        rast_samples=cfg.get("rast_samples"), eval_scene=name == "eval")
    for _ in range(3):  # warm: the last backward's records are kept
        wl.forward().backward()
        torch.cuda.synchronize()
    buf = np.zeros((1 << 16) * 16, dtype=np.int64)
    assert nat.load().pr_rast_bwd_prof_dump(ctypes.c_void_p(buf.ctypes.data), ctypes.c_size_t(buf.nbytes)) == 0
    rec = buf.reshape(-1, 16)
    np.save(out, rec[rec[:, 5] != 0])
    print("rast_bwd_timeline: collected", int((rec[:, 5] != 0).sum()), "tiles", flush=True)


def summarise(path):
    r = np.load(path)
    t0 = r[:, 4].min()
    st, en = (r[:, 4] - t0) / 100.0, (r[:, 5] - t0) / 100.0  # us
    dur = en - st
    slots, faces = r[:, 3], r[:, 13]
    ne = slots > 0
    first_end = en[ne].min()
    print(f"{path}: tiles {len(r)} ({ne.sum()} non-empty)  span {en.max():.1f} us  "
          f"(CUs seen: {len(np.unique(r[:, 6] & 0xf00007f00))})")
    print(f"  non-empty tiles started at t = 0 (before the first non-empty tile ended, {first_end:.1f} us): "
          f"{(ne & (st < first_end)).sum()};  within 2 us: {(ne & (st < 2.0)).sum()};  "
          f"last non-empty start {st[ne].max():.1f} us")
    heavy = slots >= HEAVY
    if heavy.any():
        print(f"  heavy tiles (>= {HEAVY} slots): {heavy.sum()}  last start {st[heavy].max():.1f} us  "
              f"last end {en[heavy].max():.1f} us")
    ph = r[:, 7:12].astype(np.float64)
    share = ph / np.maximum(ph.sum(1, keepdims=True), 1.0) * dur[:, None]
    for lo, hi in [(0, 1), (1, 256), (256, 512), (512, HEAVY), (HEAVY, 1 << 20)]:
        m = (slots >= lo) & (slots < hi)
        if m.any():
            print(f"  slots [{lo:3d},{min(hi, 9999):4d}): {m.sum():5d} tiles  faces {faces[m].mean():5.1f}  rounds "
                  f"{r[m, 12].mean():.2f}  dur {dur[m].mean():5.1f} (max {dur[m].max():5.1f})  start {st[m].mean():5.1f} "
                  f"(max {st[m].max():5.1f})  setup/scan/grad/transpose/flush us {share[m].mean(0).round(2).tolist()}")
    for i in np.argsort(-en)[:4]:
        print(f"  late tile {r[i, 0]},{r[i, 1]} slots {slots[i]} faces {faces[i]} start {st[i]:.1f} end {en[i]:.1f}")
    tot = float(slots.sum())
    nz, nd = (r[:, 14] & 0xffffffff).sum(), (r[:, 14] >> 32).sum()
    nb, none = (r[:, 15] & 0xffffffff).sum(), (r[:, 15] >> 32).sum()
    if tot:
        print(f"  valid slots {int(tot)}: d zbuf non-zero {nz / tot:.3f}  d dists {nd / tot:.3f}  d bary {nb / tot:.3f}  "
              f"all zero {none / tot:.3f}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "collect":
        collect(sys.argv[2])
    else:
        for p in sys.argv[1:]:
            summarise(p)
