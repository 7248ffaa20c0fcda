"""Block orders of the blend kernels' static grid, checked on the host (pr_blend_block_order: the
function the kernels call, no GPU).

Bijection: every order is a permutation of each image's blocks, and the identity where the shape
cannot take it.

Balance: on the bench frame's valid-slot counts (tests/golden/blend_order_counts.npz, written by
tests/golden/gen_blend_order_counts.py from the CPU oracle) under the dealing of workgroups that
MI355X shows -- dispatch index i goes to XCD i % 8 and there to CU (i / 8) % 32 -- the rotated
order loads every XCD and CU about alike wherever the object lies in the frame, and the linear
and centre-out orders do not (the fixture can tell them apart).  A block's work is its entries:
valid slots + 1 over its non-empty pixels.
"""
import os

import numpy as np
import pytest

from pertrenderer_amd import _native as nat

LINEAR, CENTRE_OUT, ROTATED = nat.BLEND_ORDER_LINEAR, nat.BLEND_ORDER_CENTRE_OUT, nat.BLEND_ORDER_ROTATED
SHAPES = [(3, 3), (6, 10), (24, 32), (50, 24), (256, 256), (512, 512), (100, 100)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blend_order_counts.npz")


def tiles_rows(W, PB):
    return W % PB == 0 and W // PB >= 2


@pytest.mark.parametrize("PB", [1, 2, 4, 8, 16, 32])
@pytest.mark.parametrize("H,W", SHAPES)
def test_rotated_order_is_a_bijection_per_image(H, W, PB):
    for N in (1, 3, 16):
        blocks, taken = nat.blend_block_order(N, H, W, PB, ROTATED)
        nb = (N * H * W + PB - 1) // PB
        assert blocks.shape == (nb,)
        if not tiles_rows(W, PB):  # blocks do not tile image rows (or a row is one block): linear
            assert taken == LINEAR
            np.testing.assert_array_equal(blocks, np.arange(nb, dtype=np.int32))
            continue
        assert taken == ROTATED
        bpi = H * W // PB
        per_image = blocks.reshape(N, bpi).astype(np.int64)
        # every image's dispatch indices take exactly that image's blocks, in the same order
        np.testing.assert_array_equal(np.sort(per_image, axis=1), np.arange(bpi)[None] + bpi * np.arange(N)[:, None])
        np.testing.assert_array_equal(per_image - bpi * np.arange(N)[:, None], np.broadcast_to(per_image[0], (N, bpi)))
        # ... and stay in their block row
        C = W // PB
        np.testing.assert_array_equal(per_image[0] // C, np.arange(bpi) // C)
        assert (per_image[0] != np.arange(bpi)).any()


@pytest.mark.parametrize("PB", [1, 2, 4, 8, 16, 32])
@pytest.mark.parametrize("H,W", SHAPES)
def test_linear_and_centre_out_orders(H, W, PB):
    for N in (1, 3, 16):
        nb = (N * H * W + PB - 1) // PB
        blocks, taken = nat.blend_block_order(N, H, W, PB, LINEAR)
        assert taken == LINEAR
        np.testing.assert_array_equal(blocks, np.arange(nb, dtype=np.int32))
        blocks, taken = nat.blend_block_order(N, H, W, PB, CENTRE_OUT)
        if (H * W) % PB:
            assert taken == LINEAR
            np.testing.assert_array_equal(blocks, np.arange(nb, dtype=np.int32))
        else:
            assert taken == CENTRE_OUT
            bpi = H * W // PB
            np.testing.assert_array_equal(np.sort(blocks.reshape(N, bpi), axis=1),
                                          np.arange(bpi)[None] + bpi * np.arange(N)[:, None])


def test_block_order_argument_checks():
    lib = nat.load()
    out = np.zeros(16, dtype=np.int32)
    args = lambda *a: lib.pr_blend_block_order(*a, out.ctypes.data, out.size, None)  # noqa: E731
    assert args(1, 4, 4, 1, ROTATED) == 0
    assert args(0, 4, 4, 1, ROTATED) != 0
    assert args(1, 4, 4, 0, ROTATED) != 0
    assert args(1, 4, 4, 1, 3) != 0
    assert args(1, 4, 4, 2, ROTATED) != 0  # 8 blocks, 16 offered
    assert lib.pr_blend_block_order(1, 4, 4, 1, ROTATED, None, 16, None) != 0
    assert lib.pr_blend_block_order(1, 1 << 16, 1 << 16, 1, ROTATED, out.ctypes.data, 1 << 32, None) != 0


# ---------------------------------------------------------------- balance under the dealing model
@pytest.fixture(scope="module")
def frames():
    c = np.load(GOLDEN)["counts"]
    assert c.shape == (256, 256) and c.dtype == np.uint8
    return {"centred": c, "rolled (40, 60)": np.roll(c, (40, 60), (0, 1)), "rolled (0, 100)": np.roll(c, (0, 100), (0, 1)),
            "transposed, rolled (70, 0)": np.roll(c.T, (70, 0), (0, 1))}


def dealt(frame, PB, order):
    """(per-XCD max / mean, per-CU max / mean, per-CU min / mean) of the entries of `frame`'s
    PB-pixel blocks, dispatched in `order`."""
    H, W = frame.shape
    f = frame.astype(np.int64)
    entries = np.where(f > 0, f + 1, 0).reshape(-1, PB).sum(1)
    blocks, taken = nat.blend_block_order(1, H, W, PB, order)
    assert taken == order
    work = entries[blocks]
    i = np.arange(work.size)
    xcd = np.bincount(i % 8, work, 8)
    cu = np.bincount((i % 8) * 32 + (i // 8) % 32, work, 256)
    return xcd.max() / xcd.mean(), cu.max() / cu.mean(), cu.min() / cu.mean()


@pytest.mark.parametrize("PB", [16, 32])
def test_rotated_order_balances_xcds_and_cus(frames, PB):
    for name, frame in frames.items():
        x, cmax, cmin = dealt(frame, PB, ROTATED)
        print(f"PB {PB} {name}: per XCD max/mean {x:.3f}, per CU max/mean {cmax:.2f} min/mean {cmin:.2f}")
        assert x <= 1.05, (name, x)
        assert cmax <= 1.35, (name, cmax)
        assert cmin >= 0.5, (name, cmin)


def test_fixture_tells_the_old_orders_apart(frames):
    # the bench frame has DESIGN.md's 2189 non-empty 16-pixel blocks
    assert (frames["centred"].reshape(-1, 16).sum(1) > 0).sum() == 2189
    assert dealt(frames["centred"], 16, LINEAR)[0] >= 1.3           # the backward's order so far
    assert dealt(frames["rolled (40, 60)"], 32, CENTRE_OUT)[0] >= 1.5  # the single-frame forward's
