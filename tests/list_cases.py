"""The planes and the references of the list tests ("Plane-by-plane tests of the
lists"): what k_aa_mark and the binning block of k_rates_render must make of a plane of bytes, as
sequential definitions in numpy, and the seeded families of planes built for the places where
those kernels can go wrong: the neighbour across a 64-lane boundary, across a 256-column tile,
across a multiple of 8 rows, the threshold itself, max - min against a difference from the centre,
each channel, the last partial chunk of a rate map.  Nothing here comes from the code under test;
tests/test_list_cases.py ties the references to rc.edge_mask, rc.rates_compose and plain loops
and asserts that the families hold the edges they were built for."""
import itertools

import numpy as np

U8, U32, I64 = np.uint8, np.uint32, np.int64

THRESHOLDS = (1, 2, 16, 128, 255)
MARK_BLOCK, MARK_ROWS, WAVE = 256, 8, 64     # k_aa_mark: columns a workgroup, rows a wave, lanes
RATE_CHUNK, TILE = 2048, 16                  # binning: pixels a chunk; the grid's 16 x 16 tiles
RATES, INVALID = (0, 1, 2, 4, 8), (3, 5, 7, 16, 255)


# -------------------------------------------------------------------------- references --
def mark_ref(img, t):
    """The edge mask by its definition: [..., H, W] bool, true where some channel's max - min over
    the 3 x 3 window centred on the pixel, clipped to the image, is >= t.  img: [..., H, W, 3]
    uint8; t: an int, or one per leading index."""
    a = np.asarray(img)
    assert a.dtype == U8 and a.ndim >= 3 and a.shape[-1] == 3
    h, w = a.shape[-3], a.shape[-2]
    v = a.astype(np.int16)
    lo, hi = v.copy(), v.copy()
    for dy in (-1, 0, 1):
        ys = np.clip(np.arange(h) + dy, 0, h - 1)    # a clipped window: the row taken twice
        for dx in (-1, 0, 1):
            xs = np.clip(np.arange(w) + dx, 0, w - 1)
            n = v[..., ys, :, :][..., xs, :]
            np.minimum(lo, n, out=lo)
            np.maximum(hi, n, out=hi)
    t = np.asarray(t)
    return (hi - lo).max(axis=-1) >= t.reshape(t.shape + (1, 1))


def mark_loop(img, t):
    """mark_ref for one image as a plain loop over pixels, windows and channels."""
    h, w = img.shape[:2]
    out = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            con = 0
            for c in range(3):
                vals = [int(img[yy, xx, c]) for yy in range(max(y - 1, 0), min(y + 2, h))
                        for xx in range(max(x - 1, 0), min(x + 2, w))]
                con = max(con, max(vals) - min(vals))
            out[y, x] = con >= t
    return out


def bin_masks(maps):
    """The binning by its definition, for one map [H, W] or a batch [B, H, W]: (m2, m4, m8, cnt)
    with the flattened masks [..., P] of the rate-2, rate-4 and rate-8 pixels and cnt [..., 5] =
    their three sums, the rate-1 pixels and the bytes that are no rate."""
    r = np.asarray(maps)
    assert r.dtype == U8 and r.ndim >= 2
    r = r.reshape(r.shape[:-2] + (-1,))
    m2, m4, m8 = r == 2, r == 4, r == 8
    none = ~(m2 | m4 | m8 | (r == 1) | (r == 0))
    cnt = np.stack([m.sum(axis=-1, dtype=I64) for m in (m2, m4, m8, r == 1, none)], axis=-1)
    return m2, m4, m8, cnt


def bin_ref(rates):
    """bin_masks of one map as index sets: (idx2, idx4, idx8, cnt), the sorted pixel indices of
    the three lists and the five counts."""
    m2, m4, m8, cnt = bin_masks(np.asarray(rates).reshape(1, -1))
    return np.flatnonzero(m2), np.flatnonzero(m4), np.flatnonzero(m8), cnt


def differing_neighbours(img):
    """Per direction (dx, dy) != (0, 0): [..., H, W] bool, true where the neighbour at (x + dx,
    y + dy) is inside the image and differs from the pixel in some channel."""
    a = np.asarray(img)
    h, w = a.shape[-3], a.shape[-2]
    out = {}
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            d = np.zeros(a.shape[:-1], bool)
            y0, y1, x0, x1 = max(0, -dy), h - max(0, dy), max(0, -dx), w - max(0, dx)
            if y1 > y0 and x1 > x0:
                d[..., y0:y1, x0:x1] = (a[..., y0:y1, x0:x1, :] !=
                                        a[..., y0 + dy:y1 + dy, x0 + dx:x1 + dx, :]).any(axis=-1)
            out[dx, dy] = d
    return out


def lone_crossings(img, mask):
    """How many flagged pixels have exactly one differing neighbour, and have it across a boundary
    of the kernel's layout: {"x64-": n, "x64+": n, "x256-": n, "x256+": n, "y8-": n, "y8+": n}; -
    is a neighbour at the smaller coordinate.  Such a pixel is flagged for that neighbour alone."""
    d = differing_neighbours(img)
    only = sum(v.astype(np.int8) for v in d.values()) == 1
    h, w = mask.shape[-2:]
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    n = dict.fromkeys(("x64-", "x64+", "x256-", "x256+", "y8-", "y8+"), 0)
    for (dx, dy), v in d.items():
        hit = mask & only & v
        for step, axis, c, dc in ((WAVE, "x", x, dx), (MARK_BLOCK, "x", x, dx), (MARK_ROWS, "y", y, dy)):
            if dc:
                cross = ((c + dc) // step != c // step) & np.ones((h, w), bool)
                n[f"{axis}{step}{'-' if dc < 0 else '+'}"] += int((hit & cross).sum())
    return n


# ------------------------------------------------------------------------ mark families --
def base_of(rng, t):
    """Three flat channel values with room for + t above them; 0 for t = 255."""
    return np.zeros(3, I64) if t == 255 else rng.integers(0, 256 - t, size=3)


def shapes_upto(n):
    """Every (W, H) with W * H <= n."""
    return [(w, h) for w in range(1, n + 1) for h in range(1, n // w + 1)]


def mark_small(t, w, h, k):
    """Every image of w x h over {base, base + t - 1, base + t} in channel k % 3, the other two
    channels flat: [B, h, w, 3]."""
    rng = np.random.default_rng(1000 + 10 * t + k)
    base = base_of(rng, t)
    ch = k % 3
    alpha = sorted({int(base[ch]), int(base[ch]) + t - 1, int(base[ch]) + t})
    vals = np.array(list(itertools.product(alpha, repeat=w * h)), I64)
    img = np.broadcast_to(base, (len(vals), h, w, 3)).copy()
    img[..., ch] = vals.reshape(-1, h, w)
    return img.astype(U8)


SPIKE_W = (1, 2, 3, 63, 64, 65, 127, 129, 255, 256, 257, 511, 513)
SPIKE_H = (1, 2, 7, 8, 9, 15, 16, 17)


def spike_lattice(t, w, h, phases=range(16), seed=0):
    """Flat images with single-pixel spikes on a 4 x 4 lattice, one image a phase (px, py) =
    (phase % 4, phase // 4).  The spike of lattice cell (i, j) has height t or t - 1 by the
    parity of i + j + phase and stands in channel (i + 2 * j + phase) % 3.  Returns the images
    [B, h, w, 3] and full [B, h, w], the full-height spikes.  No 3 x 3 window holds two spikes, so
    the expected mask is the clipped 3 x 3 blocks of the full-height spikes (nothing in a 1 x 1
    image, whose only window is the spike alone): spike_mask."""
    rng = np.random.default_rng(2000 + 10 * t + seed)
    phases = list(phases)
    base = base_of(rng, t)
    img = np.broadcast_to(base, (len(phases), h, w, 3)).copy()
    full = np.zeros((len(phases), h, w), bool)
    for b, ph in enumerate(phases):
        ys, xs = np.arange(ph // 4, h, 4), np.arange(ph % 4, w, 4)
        if not len(ys) or not len(xs):
            continue
        yy, xx = np.meshgrid(ys, xs, indexing="ij")
        i, j = xx // 4, yy // 4
        high = (i + j + ph) % 2 == 0
        ch = (i + 2 * j + ph) % 3
        img[b, yy, xx, ch] += np.where(high, t, t - 1)
        full[b, yy, xx] = high
    return img.astype(U8), full


def spike_mask(full):
    """The clipped 3 x 3 blocks of the spikes in full [..., H, W]."""
    h, w = full.shape[-2:]
    if h * w == 1:
        return np.zeros_like(full)
    p = np.zeros(full.shape[:-2] + (h + 2, w + 2), bool)
    for dy in range(3):
        for dx in range(3):
            p[..., dy:dy + h, dx:dx + w] |= full
    return p[..., 1:-1, 1:-1]


SPLIT_W, SPLIT_H = 322, 26


def split_contrast(t, flip):
    """One 322 x 26 image a threshold: a flat image with triples (lo, centre, hi) in a line, the
    centre at the flat value v, one neighbour at v + ceil(t / 2) and the opposite one at v -
    floor(t / 2) (flip: the other way round), so that max - min over the centre's window is t and
    no pixel differs from the centre by t (t >= 2).  Horizontal triples have their centre at x =
    64 k - 1 and at 64 k for every k up to 320 (the pair lies across a wave's edge, and at 256
    across a workgroup's); vertical ones at y = 8 k - 1 and 8 k; diagonal ones at the corners where
    x = 64 k meets y = 8.  The channel cycles.  Returns the image and the centres [(x, y)]."""
    rng = np.random.default_rng(3000 + 10 * t + flip)
    up, down = (t + 1) // 2, t // 2
    base = np.zeros(3, I64) + down if t == 255 else rng.integers(down, 256 - up, size=3)
    img = np.broadcast_to(base, (SPLIT_H, SPLIT_W, 3)).copy()
    centres, k = [], 0

    def triple(x, y, dx, dy):
        nonlocal k
        ch = k % 3
        a, b = (up, -down) if (flip + k) % 2 == 0 else (-down, up)
        img[y - dy, x - dx, ch] += a
        img[y + dy, x + dx, ch] += b
        centres.append((x, y))
        k += 1

    for xb in range(WAVE, SPLIT_W - 1, WAVE):     # 64, 128, 192, 256, 320
        triple(xb - 1, 3, 1, 0)
        triple(xb, 20, 1, 0)
    for n, yb in enumerate((8, 16)):
        triple(10 + 20 * n, yb - 1, 0, 1)
        triple(100 + 20 * n, yb, 0, 1)
    triple(WAVE, 8, 1, 1)              # the pair at (63, 7) and (65, 9)
    triple(2 * WAVE - 1, 8, 1, -1)     # at (126, 9) and (128, 7)
    triple(MARK_BLOCK, 12, 1, 1)       # rows 11 .. 13 of the second workgroup column
    return img.astype(U8), centres


NOISE_P = (0.5, 0.47, 0.03)   # base, base + t - 1, base + t: a window of 9 holds a base + t in some
                              # channel with probability 1 - 0.97^27 = 0.56 (0.42 where it holds 6)
NOISE_SHAPES = ((65, 9), (129, 17), (257, 9), (300, 20), (513, 17))


def near_threshold_noise(t, w, h, seed=0):
    """One w x h image whose pixels are base, base + t - 1 or base + t per channel (NOISE_P)."""
    rng = np.random.default_rng(4000 + 10 * t + seed)
    base = base_of(rng, t)
    pick = rng.choice(3, size=(h, w, 3), p=NOISE_P)
    return (base + np.array([0, t - 1, t])[pick]).astype(U8)


EXTREME_SHAPES = ((2, 1), (1, 2), (65, 9), (257, 17), (513, 17))


def flat_image(t, w, h):
    rng = np.random.default_rng(5000 + t)
    return np.broadcast_to(rng.integers(0, 256, size=3).astype(U8), (h, w, 3)).copy()


def checkerboard(w, h):
    """0 and 255 in every channel by the parity of x + y: every pixel of an image of more than one
    pixel has the full range in its window."""
    y, x = np.mgrid[:h, :w]
    return np.repeat((((x + y) % 2) * 255).astype(U8)[:, :, None], 3, axis=2)


STRIPS = ((8195, 3), (3, 4099))


# --------------------------------------------------------- designed lists for the entries --
def line_image(n, t=16):
    """An H = 1 image with exactly n >= 2 flagged pixels at threshold t: a step edge flags the 2
    pixels beside it and a lone spike 3, and n = 2 a + 3 b.  Features are 4 flat pixels apart."""
    assert n >= 2
    b = n % 2 + 2 * ((n - 3 * (n % 2)) // 12)
    a = (n - 3 * b) // 2
    assert a >= 0 and 2 * a + 3 * b == n
    px, level = [], 60
    kinds = ["step"] * a + ["spike"] * b
    np.random.default_rng(6000 + n).shuffle(kinds)
    px += [level] * 4
    for kind in kinds:
        if kind == "step":
            level = 60 + t if level == 60 else 60
            px += [level] * 5
        else:
            px += [level + t] + [level] * 4
    img = np.zeros((1, len(px), 3), U8)
    img[0, :, 0], img[0, :, 1], img[0, :, 2] = 33, px, 200
    return img


def step_image(w, h, t=16):
    """A vertical step at x = 64 and a horizontal one at y = 8, each t high, in two channels."""
    img = np.zeros((h, w, 3), U8)
    img[:] = (90, 140, 20)
    img[:, WAVE:, 0] += t
    img[MARK_ROWS:, :, 2] += t
    return img


# ---------------------------------------------------------------------- binning families --
def bin_small(w, h):
    """Every map of w x h over {0, 1, 2, 4, 8, 3}: [B, h, w]."""
    return np.array(list(itertools.product((0, 1, 2, 4, 8, 3), repeat=w * h)), U8).reshape(-1, h, w)


BIN_NWG = (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 72, 73)


def tiles_of(w, h):
    return ((w + TILE - 1) // TILE) * ((h + TILE - 1) // TILE)


def bin_shapes():
    """(W, H) of the random maps: every workgroup count of BIN_NWG as a wide image (one row of
    tiles, the last tile and the last row partial) and as tall ones of W = 1 .. 17 (two columns of
    tiles at W = 17, so the even counts there); and pixel counts one below, at and one above
    multiples of 2 048."""
    out = []
    for k, n in enumerate(BIN_NWG):
        out.append((TILE * n - k % TILE, TILE - k % 3))
        for w in range(1, 18):
            cols = 2 if w > TILE else 1
            if n % cols == 0:
                out.append((w, TILE * (n // cols) - (w + k) % TILE))
    out += [(2047, 1), (2048, 1), (2049, 1), (128, 16), (23, 89), (3, 683), (4095, 1), (64, 64),
            (4097, 1), (1, 2047), (1, 2049), (17, 241)]
    return list(dict.fromkeys(out))


def missing_duty(w, h):
    """True when the map's last chunk is partial, holds pixels, and the workgroup whose turn it
    would be does not exist (so the first of the chunk bins it)."""
    nwg = tiles_of(w, h)
    chunk = (nwg - 1) // 8
    return nwg % 8 != 0 and chunk * 8 + chunk % 8 >= nwg and chunk * RATE_CHUNK < w * h


def random_map(w, h, seed):
    """Bytes of the five rates and the five invalid values; the mix differs with the seed."""
    rng = np.random.default_rng(7000 + 31 * w + h + 7919 * seed)
    alpha = np.array(RATES + INVALID, U8)
    p = 0.5 * rng.dirichlet(np.ones(len(alpha)) * (0.6 if seed % 2 else 3.0)) + 0.05
    return alpha[rng.choice(len(alpha), size=(h, w), p=p)]


BIN_EXTREME_SHAPES = ((1, 1), (33, 70), (144, 16), (130, 33))


def bin_extremes(w, h):
    """{name: map}: one rate everywhere (2 and 8 each fill the buffer they share), the two halves
    (the lists meet exactly), interleaved, and nothing to list."""
    n = w * h
    i = np.arange(n)
    out = {f"all{r}": np.full(n, r, U8) for r in (0, 1, 2, 4, 8, 5, 255)}
    out["half28"] = np.where(i < n // 2, 2, 8).astype(U8)
    out["half82"] = np.where(i < (n + 1) // 2, 8, 2).astype(U8)
    out["odd28"] = np.where(i % 2 == 0, 2, 8).astype(U8)
    return {k: v.reshape(h, w) for k, v in out.items()}


def counted_map(w, h, counts, seed):
    """A map with exactly counts = {rate: n} pixels of those rates at seeded places, 0 elsewhere."""
    rng = np.random.default_rng(8000 + seed)
    at = rng.permutation(w * h)
    m, k = np.zeros(w * h, U8), 0
    for rate, n in counts.items():
        m[at[k:k + n]] = rate
        k += n
    assert k <= w * h
    return m.reshape(h, w)
