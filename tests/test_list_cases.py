"""The list tests' references and families on the CPU (tests/list_cases.py; DESIGN.md, "Plane-by-
plane tests of the lists"): mark_ref against rc.edge_mask and a plain loop, bin_ref against
rc.rates_compose's classes, and the edges every family was built for, counted with numpy alone, so
that a family that lost them fails here and not silently on the GPU."""
import itertools

import numpy as np
import pytest

import list_cases as lc
from helpers import rc

U8 = np.uint8


# -------------------------------------------------------------------------- references --
def test_mark_ref_on_every_tiny_image():
    """Every image of every shape of <= 6 pixels over a 3-value alphabet in one channel (two
    alphabets), at the three thresholds that separate its values: the definition, the plain loop
    and rc.edge_mask agree on each of the 22 320."""
    n = 0
    for w, h in lc.shapes_upto(6):
        for ch, alpha in ((0, (10, 11, 13)), (2, (0, 254, 255))):
            vals = np.array(list(itertools.product(alpha, repeat=w * h)), U8)
            img = np.full((len(vals), h, w, 3), 40, U8)
            img[..., ch] = vals.reshape(-1, h, w)
            ts = sorted({b - a for a in alpha for b in alpha if b > a})
            for t in ts:
                ref = lc.mark_ref(img, t)
                for b in range(len(img)):
                    np.testing.assert_array_equal(ref[b], rc.edge_mask(img[b], t))
                    np.testing.assert_array_equal(ref[b], lc.mark_loop(img[b], t))
                    n += 1
    # 3 + 2 * 9 + 2 * 27 + 3 * 81 + 2 * 243 + 4 * 729 = 3 720 images an alphabet, three thresholds each
    assert n == 2 * 3 * 3720


def test_mark_ref_on_seeded_images():
    rng = np.random.default_rng(5)
    for (w, h), t in zip([(1, 1), (7, 3), (33, 17), (65, 9), (3, 40)], lc.THRESHOLDS):
        img = rng.integers(0, 256, size=(h, w, 3), dtype=U8)
        near = lc.near_threshold_noise(t, w, h)
        for a in (img, near):
            np.testing.assert_array_equal(lc.mark_ref(a, t), rc.edge_mask(a, t))
            np.testing.assert_array_equal(lc.mark_ref(a, t), lc.mark_loop(a, t))
    batch = rng.integers(0, 256, size=(5, 9, 11, 3), dtype=U8)
    got = lc.mark_ref(batch, np.array(lc.THRESHOLDS))   # one threshold an image
    for b, t in enumerate(lc.THRESHOLDS):
        np.testing.assert_array_equal(got[b], rc.edge_mask(batch[b], t))


def test_bin_ref_is_rates_compose_classes():
    """The index sets are the pixels rates_compose takes from images[s]; the invalid bytes are
    the ones it refuses."""
    for seed, (w, h) in enumerate([(1, 1), (7, 3), (33, 17), (144, 16)]):
        m = lc.random_map(w, h, seed)
        i2, i4, i8, cnt = lc.bin_ref(m)
        valid = np.where(np.isin(m, lc.RATES), m, 0).astype(U8)
        base = np.zeros((h, w, 3), U8)
        images = {s: np.full((h, w, 3), s, U8) for s in (1, 2, 4, 8)}
        out = rc.rates_compose(base, images, valid)[:, :, 0].ravel()
        for s, idx in ((2, i2), (4, i4), (8, i8)):
            np.testing.assert_array_equal(idx, np.flatnonzero(out == s))
        assert cnt.tolist() == [len(i2), len(i4), len(i8), int((out == 1).sum()),
                                int((~np.isin(m, lc.RATES)).sum())]
        if cnt[4]:
            with pytest.raises(ValueError):
                rc.rates_compose(base, images, m)
        loop = [sum(1 for v in m.ravel().tolist() if v == s) for s in (2, 4, 8, 1)]
        assert cnt[:4].tolist() == loop


# ------------------------------------------------------------------------ mark families --
def test_small_family_sizes():
    shapes = lc.shapes_upto(8)
    assert len(shapes) == 20 and max(w * h for w, h in shapes) == 8
    img = lc.mark_small(16, 4, 2, 1)
    assert img.shape == (3 ** 8, 2, 4, 3) and len(np.unique(img[..., 1])) == 3
    assert lc.mark_small(1, 8, 1, 0).shape[0] == 2 ** 8      # base + t - 1 is base
    m = lc.mark_ref(img, 16)
    assert 0 < m.sum() < m.size and m[0].sum() == 0


@pytest.mark.parametrize("t", lc.THRESHOLDS)
def test_spike_lattice_mask_is_the_blocks(t):
    """By construction the mask is the clipped 3 x 3 blocks of the full-height spikes; the family
    holds every crossing it was built for, and lone t - 1 spikes."""
    crossings = dict.fromkeys(("x64-", "x64+", "x256-", "x256+", "y8-", "y8+"), 0)
    edges = dict.fromkeys(("x0", "x1", "y0", "y1", "c00", "c01", "c10", "c11"), 0)
    low_alone = images = 0
    for w in lc.SPIKE_W:
        for h in lc.SPIKE_H:
            img, full = lc.spike_lattice(t, w, h)
            want = lc.spike_mask(full)
            ref = lc.mark_ref(img, t)
            np.testing.assert_array_equal(ref, want, err_msg=f"{w}x{h} t{t}")
            images += len(img)
            if w * h == 1:
                assert not ref.any()
                continue
            for k, v in lc.lone_crossings(img, ref).items():
                crossings[k] += v
            f = full
            for k, v in (("x0", f[:, :, 0]), ("x1", f[:, :, -1]), ("y0", f[:, 0, :]), ("y1", f[:, -1, :]),
                         ("c00", f[:, 0, 0]), ("c01", f[:, 0, -1]), ("c10", f[:, -1, 0]), ("c11", f[:, -1, -1])):
                edges[k] += int(v.sum())
            if t > 1:   # a t - 1 spike with nothing flagged in its block
                low = (img != img.min(axis=(1, 2), keepdims=True)).any(axis=-1) & ~full
                low_alone += int((low & ~lc.spike_mask(ref)).sum())
    assert images == 16 * len(lc.SPIKE_W) * len(lc.SPIKE_H)
    assert all(v > 0 for v in crossings.values()), crossings
    assert all(v > 0 for v in edges.values()), edges
    assert t == 1 or low_alone > 0


def test_spike_lattice_against_edge_mask():
    """720 images of the family (nine shapes, every phase, every threshold) against rc.edge_mask."""
    n = 0
    for w, h in [(1, 1), (2, 1), (3, 2), (63, 7), (65, 9), (129, 8), (257, 2), (256, 17), (513, 1)]:
        for t in lc.THRESHOLDS:
            img, full = lc.spike_lattice(t, w, h)
            want = lc.spike_mask(full)
            for b in range(16):
                np.testing.assert_array_equal(rc.edge_mask(img[b], t), want[b])
                n += 1
    assert n == 720


@pytest.mark.parametrize("t", lc.THRESHOLDS)
def test_split_contrast_centres(t):
    for flip in (0, 1):
        img, centres = lc.split_contrast(t, flip)
        ref = lc.mark_ref(img, t)
        np.testing.assert_array_equal(ref, rc.edge_mask(img, t))
        assert len(centres) == 17
        xs, ys = {x for x, _ in centres}, {y for _, y in centres}
        assert {63, 64, 127, 128, 191, 192, 255, 256, 319, 320} <= xs and {7, 8, 15, 16} <= ys
        v = img.astype(int)
        for x, y in centres:
            assert ref[y, x], (t, flip, x, y)
            win = v[y - 1:y + 2, x - 1:x + 2]
            assert (win.max(axis=(0, 1)) - win.min(axis=(0, 1))).max() == t
            if t >= 2:   # a difference from the centre would miss it
                assert np.abs(win - v[y, x]).max() < t


@pytest.mark.parametrize("t", lc.THRESHOLDS)
def test_noise_share(t):
    for k, (w, h) in enumerate(lc.NOISE_SHAPES + lc.STRIPS):
        img = lc.near_threshold_noise(t, w, h, k)
        share = lc.mark_ref(img, t).mean()
        assert 0.2 <= share <= 0.8, (t, w, h, share)
        assert len(np.unique(img)) <= 9


def test_extremes_and_lines():
    for w, h in lc.EXTREME_SHAPES:
        for t in lc.THRESHOLDS:
            assert not lc.mark_ref(lc.flat_image(t, w, h), t).any()
            assert lc.mark_ref(lc.checkerboard(w, h), t).all()
    for n in (2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513):
        img = lc.line_image(n)
        assert img.shape[0] == 1 and int(lc.mark_ref(img, 16).sum()) == n
        assert int(lc.mark_ref(img, 17).sum()) == 0
    st = lc.mark_ref(lc.step_image(129, 17), 16)
    assert st[:, 63:65].all() and st[7:9, :].all() and st.sum() == 2 * 17 + 2 * 129 - 4


# ---------------------------------------------------------------------- binning families --
def test_bin_shapes_hold_their_edges():
    shapes = lc.bin_shapes()
    assert len(set(shapes)) == len(shapes)
    nwg = {lc.tiles_of(w, h) for w, h in shapes}
    assert set(lc.BIN_NWG) <= nwg
    for n in lc.BIN_NWG:   # wide and tall, every W = 1 .. 16 and, for the even counts, 17
        ws = {w for w, h in shapes if lc.tiles_of(w, h) == n}
        assert set(range(1, 17)) <= ws and (n % 2 or 17 in ws), n
        assert any(h <= lc.TILE and w > lc.TILE * (n - 1) for w, h in shapes), n
    missing = [(w, h) for w, h in shapes if lc.missing_duty(w, h)]
    assert {lc.tiles_of(w, h) for w, h in missing} >= {9, 17, 73}
    held = set()   # workgroup counts where the chunk nobody would bin holds all three lists
    for w, h in missing:
        last = lc.random_map(w, h, 0).ravel()[(lc.tiles_of(w, h) - 1) // 8 * lc.RATE_CHUNK:]
        if all((last == s).any() for s in (2, 4, 8)):
            held.add(lc.tiles_of(w, h))
    assert held >= {9, 17, 73}, held
    px = {w * h for w, h in shapes}
    assert {2047, 2048, 2049, 4095, 4096, 4097} <= px
    for seed in (0, 1):
        assert set(np.unique(lc.random_map(144, 16, seed))) == set(lc.RATES + lc.INVALID)


def test_bin_small_and_extremes():
    assert len(lc.shapes_upto(6)) == 14
    assert lc.bin_small(3, 2).shape == (6 ** 6, 2, 3)
    for w, h in lc.BIN_EXTREME_SHAPES:
        ex = lc.bin_extremes(w, h)
        n = w * h
        assert lc.bin_ref(ex["all2"])[3].tolist() == [n, 0, 0, 0, 0]
        assert lc.bin_ref(ex["all8"])[3].tolist() == [0, 0, n, 0, 0]
        assert lc.bin_ref(ex["all255"])[3].tolist() == [0, 0, 0, 0, n]
        for k in ("half28", "half82", "odd28"):
            c = lc.bin_ref(ex[k])[3]
            assert c[0] + c[2] == n and c[1] == c[3] == c[4] == 0 and (n == 1 or c[0] * c[2] > 0)
    m = lc.counted_map(33, 17, {2: 15, 4: 5, 8: 2}, 3)
    assert lc.bin_ref(m)[3].tolist() == [15, 5, 2, 0, 0]
