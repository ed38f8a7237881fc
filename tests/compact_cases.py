"""Cases and references of the class-map tests of the DEP compaction and the row shards (DESIGN.md,
"Class-map tests of the compaction"): shared by tests/test_compact_cases.py (CPU: the references
against the oracle's frames, the edges where the lists say they are) and tests/test_gpu_compact.py
(device against the references).  Seeded.  Nothing here comes from the kernels: segment_ref is the
sequential definition in the comment above them, written in numpy.

A class map holds 0 (ident), 1 (writer) and 2 (DEP), H rows of W pixels in scan order.  The DEP
pixels are listed in scan order; a DEP pixel starts a segment iff no DEP pixel precedes it or the
last writer before it lies after the previous DEP pixel; the segment's key is that writer, or -1."""
import functools
import itertools
import types

import numpy as np

IDENT, WRITER, DEP = 0, 1, 2
U8, I32, I64 = np.uint8, np.int32, np.int64
ROW_CHUNK = 4096          # pixels of a row per LDS chunk (kRowChunk)
SCAN_CHUNK = 2048         # rows per scan chunk (kScanBlock * kScanRows)
SEG_ORDER_MAX = 65536     # above it the queue stays in segment order
ROWSTATS = np.dtype([("ndep", "<i4"), ("nstart", "<i4"), ("lastw", "<i8"), ("lastd", "<i8"), ("wfirst", "<i8")])


# ---------------------------------------------------------------------- the reference --
def _excl(a, op, first):
    """Exclusive scan along the last axis."""
    out = np.empty_like(a)
    out[..., 0] = first
    out[..., 1:] = op.accumulate(a, axis=-1)[..., :-1]
    return out


def segment_ref(cls):
    """The compaction of one class map [H, W] or of a batch [B, H, W], from the definition.  Works on
    the non-ident pixels only (an event list), so a sparse map of millions of pixels costs little.

    Per map (ragged, lists of arrays when batched, plain arrays for one map): dep (the DEP pixels),
    seg_start (each segment's first index into dep), seg_key, inrow (per DEP pixel: the last writer
    before it in its own row, -1 = none).  Per row [B, H]: rows (RowStats: DEP count, segment starts
    other than at the row's first DEP pixel, last writer, last DEP pixel, the last writer of the row
    before its first DEP pixel; pixels are image indices, -1 = none), row_off / row_soff (DEP pixels
    / segments before the row), row_prevw / row_prevd (last writer / DEP pixel before the row)."""
    cls = np.asarray(cls, U8)
    single = cls.ndim == 2
    if single:
        cls = cls[None]
    B, H, W = cls.shape
    P = H * W
    flat = cls.reshape(-1)
    ev = np.flatnonzero(flat).astype(I64)      # events in scan order, map after map
    c = flat[ev]
    m = ev // P
    org = m * P
    isw, isd = c == WRITER, c == DEP
    lw = np.maximum.accumulate(np.where(isw, ev, -1)) if len(ev) else ev
    ld = np.maximum.accumulate(np.where(isd, ev, -1)) if len(ev) else ev
    lw = np.where(lw >= org, lw - org, -1)                       # last writer before, in this map
    pd = np.concatenate(([-1], ld[:-1])).astype(I64)[:len(ev)]   # last DEP strictly before
    pd = np.where(pd >= org, pd - org, -1)
    d = np.flatnonzero(isd)
    dm, dp, key, dpd = m[d], ev[d] - org[d], lw[d], pd[d]
    start = (dpd < 0) | (key > dpd)
    ndep = np.bincount(dm, minlength=B).astype(I64)
    nseg = np.bincount(dm[start], minlength=B).astype(I64)
    doff = np.concatenate(([0], np.cumsum(ndep)))
    soff = np.concatenate(([0], np.cumsum(nseg)))
    di = np.arange(len(d)) - doff[dm]                            # index in its map's list
    s = np.flatnonzero(start)
    inrow = np.where(key >= (dp // W) * W, key, -1)
    # rows
    R = ev // W                                                  # row of the event, over all maps
    Rd = R[d]
    rows = np.zeros(B * H, ROWSTATS)
    rows["ndep"] = np.bincount(Rd, minlength=B * H)
    allst = np.bincount(Rd[start], minlength=B * H)
    first = np.concatenate(([True], Rd[1:] != Rd[:-1]))[:len(d)]   # the row's first DEP pixel
    rows["nstart"] = allst - np.bincount(Rd[first & start], minlength=B * H)
    for name, sel in (("lastw", isw), ("lastd", isd)):
        a = np.full(B * H, -1, I64)
        np.maximum.at(a, R[sel], ev[sel] - org[sel])
        rows[name] = a
    wf = np.full(B * H, -1, I64)
    wf[Rd[first]] = inrow[first]
    rows["wfirst"] = wf
    rows = rows.reshape(B, H)
    out = types.SimpleNamespace(
        B=B, H=H, W=W, P=P, ndep=ndep, nseg=nseg, rows=rows,
        row_off=_excl(rows["ndep"].astype(I64), np.add, 0),
        row_soff=_excl(allst.reshape(B, H).astype(I64), np.add, 0),
        row_prevw=_excl(rows["lastw"], np.maximum, -1), row_prevd=_excl(rows["lastd"], np.maximum, -1),
        dep=[dp[doff[b]:doff[b + 1]] for b in range(B)] if B < 64 else None,
        seg_start=[di[s][soff[b]:soff[b + 1]] for b in range(B)] if B < 64 else None,
        seg_key=[key[s][soff[b]:soff[b + 1]] for b in range(B)] if B < 64 else None,
        inrow=[inrow[doff[b]:doff[b + 1]] for b in range(B)] if B < 64 else None,
        # the flat lists, for padded tables of large batches
        _dm=dm, _di=di, _dp=dp, _sm=dm[s], _si=np.arange(len(s)) - soff[dm[s]], _ss=di[s], _sk=key[s])
    if single:
        for k in ("dep", "seg_start", "seg_key", "inrow"):
            setattr(out, k, getattr(out, k)[0])
        for k in ("rows", "row_off", "row_soff", "row_prevw", "row_prevd"):
            setattr(out, k, getattr(out, k)[0])
        out.ndep, out.nseg = int(ndep[0]), int(nseg[0])
    return out


def padded_tables(ref, cap, fill32, fill64):
    """dep_pix [B, cap] (int64), seg_start [B, cap] (int32), seg_key [B, cap] (int64) as a device
    buffer of cap slots a map must look: the lists, then the sentinel."""
    dep = np.full((ref.B, cap), fill64, I64)
    ss = np.full((ref.B, cap), fill32, I32)
    sk = np.full((ref.B, cap), fill64, I64)
    dep[ref._dm, ref._di] = ref._dp
    ss[ref._sm, ref._si] = ref._ss
    sk[ref._sm, ref._si] = ref._sk
    return dep, ss, sk


def segment_slow(cls):
    """The same definition as one Python loop over the pixels (small maps): (dep, seg_start, seg_key)."""
    dep, ss, sk = [], [], []
    lastw = lastd = -1
    for p, c in enumerate(np.asarray(cls).reshape(-1)):
        if c == WRITER:
            lastw = p
        elif c == DEP:
            if lastd < 0 or lastw > lastd:
                ss.append(len(dep))
                sk.append(lastw)
            dep.append(p)
            lastd = p
    return np.array(dep, I64), np.array(ss, I64), np.array(sk, I64)


def order_ref(seg_start, ndep, block_min, block_cap):
    """k_seg_order's contract: (order, counters[3], counters[14], counters[15]).  A stable sort by
    falling length bucket (32 entries a bucket, 255 the last); nlong = the segments whose bucket is
    >= ceil(block_min / 32) (at most 255), 0 when block_min is 0 or when they are more than 2 *
    block_cap.  Above SEG_ORDER_MAX segments: order None (untouched) and the three counters 0."""
    seg_start = np.asarray(seg_start, I64)
    nseg = len(seg_start)
    if nseg > SEG_ORDER_MAX:
        return None, 0, 0, 0
    ln = np.diff(np.concatenate((seg_start, [ndep])))
    bucket = np.minimum(ln >> 5, 255)
    order = np.argsort(-bucket, kind="stable")
    nlong = 0
    if block_min > 0:
        nlong = int((bucket >= min((block_min + 31) // 32, 255)).sum())
        if nlong > 2 * block_cap:
            nlong = 0
    return order, 1, nlong, nlong


def key_writers_loop(cls):
    """Phase A's key-writer filter over a map [H, W], by tests/test_layout.py's restatement of
    writer_may_key, fragment by fragment: a writer stores its carry unless a later writer of its
    8-pixel row fragment follows with no DEP pixel between them."""
    from test_layout import writer_may_key
    cls = np.asarray(cls)
    H, W = cls.shape
    keep = np.zeros((H, W), bool)
    for y in range(H):
        for x0 in range(0, W, 8):
            frag = [int(cls[y, x]) if x < W else -1 for x in range(x0, x0 + 8)]
            for l in range(8):
                if x0 + l < W and frag[l] == WRITER:
                    keep[y, x0 + l] = writer_may_key(frag, l)
    return keep


def key_writers(cls):
    """The same rule for whole maps in numpy (tests/test_compact_cases.py holds it to key_writers_loop
    on every map of the wkey family): with nw / nd the next writer / DEP pixel after x in the row, the
    writer at x stores unless nw lies in x's fragment (nw <= x | 7) with no DEP pixel before it."""
    cls = np.asarray(cls)
    H, W = cls.shape
    x = np.arange(W)[None, :]

    def next_after(mask):
        pos = np.where(mask, x, W + 8)                       # at or after x ...
        at = np.minimum.accumulate(pos[:, ::-1], axis=1)[:, ::-1]
        return np.concatenate((at[:, 1:], np.full((H, 1), W + 8)), axis=1)   # ... strictly after
    nw, nd = next_after(cls == WRITER), next_after(cls == DEP)
    return (cls == WRITER) & ((nw > (x | 7)) | (nd < nw))


# ------------------------------------------------------------------------ the families --
class Case:
    def __init__(self, label, cls):
        self.label, self.cls = label, np.ascontiguousarray(cls, U8)
        self.cls.setflags(write=False)

    @functools.cached_property
    def ref(self):
        return segment_ref(self.cls)

    @functools.cached_property
    def keep(self):
        return key_writers(self.cls)

    def __repr__(self):
        return f"{self.label} {self.cls.shape[1]}x{self.cls.shape[0]}"


def small_shapes(limit=8):
    return [(W, H) for W in range(1, limit + 1) for H in range(1, limit + 1) if W * H <= limit]


def small_batch(W, H):
    """Every map of W x H: [3 ** (W * H), H, W]."""
    n = W * H
    v = np.arange(3 ** n)
    return np.stack([(v // 3 ** k) % 3 for k in range(n)], 1).astype(U8).reshape(-1, H, W)


STRADDLE_B = (8, 64, 128, 4096, 8192)
STRADDLE_DW = (-1, 0, 1, 3, 17)
PATTERNS = np.array(list(itertools.product((0, 1, 2), repeat=6)), U8)   # on x = b - 3 .. b + 2


@functools.lru_cache(None)
def straddle_cases(b):
    """For every width: the 729 patterns across x = b, one a row in seeded order, over an ident
    background and over a sparse seeded one.  From b = 4096 on the rows are dealt to three maps of 243
    (a 8209 x 729 map has 6 M pixels): every pattern is still there, over both backgrounds."""
    out = []
    for dw in STRADDLE_DW:
        W = b + dw
        for bg in ("ident", "sparse"):
            rng = np.random.default_rng([b, dw + 1, bg == "sparse"])
            perm = rng.permutation(729)
            parts = 3 if b >= 4096 else 1
            for part in range(parts):
                rows = perm[part::parts]
                m = np.zeros((len(rows), W), U8)
                if bg == "sparse":
                    m[:] = rng.choice(3, size=m.shape, p=[0.98, 0.01, 0.01])
                for k, x in enumerate(range(b - 3, b + 3)):
                    if 0 <= x < W:
                        m[:, x] = PATTERNS[rows, k]
                c = Case(f"straddle/b{b}/W{W}/{bg}/{part}", m)
                c.b, c.patterns = b, rows
                out.append(c)
    return out


ROWS_H = (1, 2, 3, 4, 5, 7, 8, 9, 2047, 2048, 2049, 4095, 4096, 4097, 6145)
ROWS_W = (1, 3, 64, 65)
UPPER = ("writer-last", "dep-last", "neither")      # how the row before the boundary ends
LOWER = ("dep-first", "writer-dep", "no-dep")       # how the row after it begins


def _boundary_rows(W, up, lo):
    """The two rows around a scan-chunk boundary, W >= 3."""
    a, b = np.zeros(W, U8), np.zeros(W, U8)
    if up == "writer-last":
        a[0], a[W - 1] = DEP, WRITER
    elif up == "dep-last":
        a[0], a[W - 1] = WRITER, DEP
    if lo == "dep-first":
        b[0] = DEP
    elif lo == "writer-dep":
        b[0], b[1] = WRITER, DEP
    return a, b


@functools.lru_cache(None)
def rows_cases():
    out = []
    for H in ROWS_H:
        for W in ROWS_W:
            rng = np.random.default_rng([7, H, W])
            p = rng.dirichlet([1, 1, 1]) if H < 100 else np.array([0.9, 0.05, 0.05])
            out.append(Case(f"rows/{W}x{H}", rng.choice(3, size=(H, W), p=p)))
    for k in (2048, 4096):
        for W in (3, 64, 65):
            for up in UPPER:
                for lo in LOWER:
                    rng = np.random.default_rng([8, k, W, UPPER.index(up), LOWER.index(lo)])
                    m = rng.choice(3, size=(k + 3, W), p=[0.9, 0.05, 0.05]).astype(U8)
                    m[k - 1], m[k] = _boundary_rows(W, up, lo)
                    c = Case(f"rows/boundary{k}/W{W}/{up}/{lo}", m)
                    c.boundary, c.combo = k, (up, lo)
                    out.append(c)
        for W in (3, 65):   # a row of writers only before the boundary, a DEP pixel first after it
            rng = np.random.default_rng([15, k, W])
            m = rng.choice(3, size=(k + 3, W), p=[0.9, 0.05, 0.05]).astype(U8)
            m[k - 1], m[k], m[k, 0] = WRITER, IDENT, DEP
            c = Case(f"rows/boundary{k}/W{W}/writers-only/dep-first", m)
            c.writers_only = k
            out.append(c)
        for W in (1,):   # one pixel a row: the upper row IS a writer, a DEP pixel or neither
            for up, uc in zip(UPPER, (WRITER, DEP, IDENT)):
                for lo, lc in (("dep-first", DEP), ("no-dep", IDENT)):
                    rng = np.random.default_rng([9, k, uc, lc])
                    m = rng.choice(3, size=(k + 3, W), p=[0.8, 0.1, 0.1]).astype(U8)
                    m[k - 1, 0], m[k, 0] = uc, lc
                    out.append(Case(f"rows/boundary{k}/W1/{up}/{lo}", m))
        for name, v in (("writers", WRITER), ("ident", IDENT), ("dep", DEP)):
            rng = np.random.default_rng([10, k, v])
            m = rng.choice(3, size=(k + 8, 65), p=[0.9, 0.05, 0.05]).astype(U8)
            m[k - 4:k + 4] = v
            c = Case(f"rows/stretch{k}/{name}", m)
            c.stretch = (k, v)
            out.append(c)
    return out


DENSITY_SHAPES = ((33, 17), (97, 61), (333, 517), (4099, 5))


def extremes(W, H):
    alt = np.resize(np.array([WRITER, DEP], U8), W * H).reshape(H, W)
    last = np.zeros((H, W), U8)
    last[-1, -1] = DEP
    both = last.copy()
    both[0, 0] = WRITER
    return [("all-ident", np.zeros((H, W), U8)), ("all-writer", np.full((H, W), WRITER, U8)),
            ("all-dep", np.full((H, W), DEP, U8)), ("alternating", alt), ("dep-at-last", last),
            ("writer-first-dep-last", both)]


@functools.lru_cache(None)
def density_cases():
    out = []
    for W, H in DENSITY_SHAPES:
        for seed in range(3):
            rng = np.random.default_rng([11, W, H, seed])
            p = rng.dirichlet([1, 1, 1])
            out.append(Case(f"density/{W}x{H}/dirichlet{seed}", rng.choice(3, size=(H, W), p=p)))
        for name, m in extremes(W, H):
            if W * H > 1 or "first" not in name:
                out.append(Case(f"density/{W}x{H}/{name}", m))
    return out


@functools.lru_cache(None)
def many_cases():
    """512 x 257 alternating (65 792 segments) and the same with its last pairs taken out: exactly
    65 535, 65 536 and 65 537 segments (the queue's cut-over to segment order lies above 65 536)."""
    W, H = 512, 257
    alt = np.resize(np.array([WRITER, DEP], U8), W * H)
    out = [Case("many/65792", alt.reshape(H, W))]
    for n in (65535, 65536, 65537):
        m = alt.copy()
        m[2 * n:] = IDENT
        out.append(Case(f"many/{n}", m.reshape(H, W)))
    return out


NATURAL = ([(n, 64, 48) for n in ("simple", "reflection", "quadric", "example2", "example3", "quadric2",
                                  "phantom_two", "phantom_four")] +
           [(n, 96, 72) for n in ("simple", "reflection", "quadric", "example2", "example3", "quadric2",
                                  "phantom_two", "phantom_four")] +
           [("quadric", 256, 256), ("quadric", 333, 517), ("reflection", 8195, 3), ("reflection", 3, 4099)])
NATURAL_DEPTH = 6


@functools.lru_cache(None)
def natural_frame(name, W, H):
    """The oracle's frame: (scene, class map with class 3 counted as DEP, carry-in per pixel)."""
    import resolve_cases as rv
    from helpers import rc, scene_path
    scene = rc.Scene.from_file(scene_path(name))
    _, cls, cin = rv.render_cls(scene, W, H, NATURAL_DEPTH + 1)
    return scene, np.minimum(cls, DEP).reshape(H, W), cin


@functools.lru_cache(None)
def natural_cases():
    return [Case(f"natural/{n}/{W}x{H}", natural_frame(n, W, H)[1]) for n, W, H in NATURAL]


# -- k_seg_order alone: (label, seg_start, ndep, block_min, block_cap) --
ORDER_LENGTHS = (1, 31, 32, 33, 63, 64, 8159, 8160, 8161, 100000)
ORDER_NSEG = (0, 1, 255, 256, 257, 1000, 65535, 65536, 65537)
ORDER_BLOCK_MIN = (0, 1, 31, 32, 33, 256, 8160, 10000)


def _table(lengths):
    lengths = np.asarray(lengths, I64)
    return np.concatenate(([0], np.cumsum(lengths)[:-1])).astype(I32)[:len(lengths)], int(lengths.sum())


@functools.lru_cache(None)
def order_cases():
    out = []
    rng = np.random.default_rng(12)
    for nseg in ORDER_NSEG:
        big = nseg > 2000        # keep ndep small: the long tables hold three long segments only
        pool = np.array(ORDER_LENGTHS[:6] if big else ORDER_LENGTHS)
        mixed = pool[rng.integers(0, len(pool), nseg)]
        runs = np.repeat(pool[rng.permutation(len(pool))], -(-max(nseg, 1) // len(pool)))[:nseg]
        for kind, ln in (("mixed", mixed), ("runs", runs)):
            if big:
                ln = ln.copy()
                ln[[1, nseg // 2, nseg - 2]] = (8159, 8160, 100000)
            ss, ndep = _table(ln)
            for bm in ORDER_BLOCK_MIN:
                out.append((f"order/{kind}/n{nseg}/bmin{bm}", ss, ndep, bm, 1 << 20))
    # block_cap at the long count: exactly 2 * block_cap long segments, and one more
    for nlong, bm in ((8, 64), (9, 64), (64, 33), (65, 33), (2, 8160), (3, 8160)):
        ln = np.concatenate((np.full(nlong, max(bm, 32) + 31), rng.integers(1, 32, 200)))
        ss, ndep = _table(rng.permutation(ln))
        out.append((f"order/cap/long{nlong}/bmin{bm}", ss, ndep, bm, nlong // 2))
    for v in ORDER_LENGTHS:   # one segment of every length alone, and 300 of them
        for n in (1, 300):
            if v * n < 2 ** 31:
                ss, ndep = _table(np.full(n, v))
                out.append((f"order/equal/{v}x{n}", ss, ndep, 32, 1 << 20))
    return out


# -- the key writers: maps of the density and straddle (b = 8) kinds and every width 1 .. 17 --
@functools.lru_cache(None)
def wkey_cases():
    out = list(density_cases()) + list(straddle_cases(8))
    for W in range(1, 18):
        rng = np.random.default_rng([13, W])
        out.append(Case(f"wkey/W{W}", rng.choice(3, size=(37, W), p=rng.dirichlet([1, 1, 1]))))
    return out


# -- the row shards --
SHARD_G = (1, 2, 3, 5, 8, 16)
SHARD_W = (1, 7, 64, 65, 97)


def shard_heights(G):
    return sorted({h for h in (1, G - 1, G, G + 1, 2 * G + 1, 31) if h >= 1})


@functools.lru_cache(None)
def shard_cases():
    """(G, Case): per G, H and W a seeded map of the density kind; for W >= 64 also one of the
    straddle kind (the patterns across x = 64, a row each, over a sparse background)."""
    out = []
    for G in SHARD_G:
        for H in shard_heights(G):
            for W in SHARD_W:
                rng = np.random.default_rng([14, G, H, W])
                out.append((G, Case(f"shard/G{G}/{W}x{H}/density", rng.choice(3, size=(H, W), p=rng.dirichlet([1, 1, 1])))))
                if W >= 64:
                    m = rng.choice(3, size=(H, W), p=[0.9, 0.05, 0.05]).astype(U8)
                    rows = rng.permutation(729)[:H]
                    for k, x in enumerate(range(61, 67)):
                        if x < W:
                            m[:, x] = PATTERNS[rows, k]
                    out.append((G, Case(f"shard/G{G}/{W}x{H}/straddle", m)))
    return out


DEINTERLEAVE = [(G, W, H) for G in (1, 2, 3, 5, 16) for W in (4, 8, 1, 7, 97) for H in (1, G, 2 * G + 1, 31)]


# ----------------------------------------------------------------------------- the edges --
def straddle_edges(c):
    """Which of the required edges a straddle map holds, from numpy alone (a dict of counts)."""
    m, b = c.cls, c.b
    H, W = m.shape
    e = dict.fromkeys(("writer-keys-across", "first-dep-after-with-writer", "first-dep-after-without-writer",
                       "dep-continues-across", "only-writer-after-last-dep"), 0)
    for y in range(H):
        r = m[y]
        deps, ws = np.flatnonzero(r == DEP), np.flatnonzero(r == WRITER)
        if b < W and r[b] == DEP and r[b - 1] == WRITER:
            e["writer-keys-across"] += 1
        if len(deps) and deps[0] == b:
            e["first-dep-after-with-writer" if len(ws) and ws[0] < b else "first-dep-after-without-writer"] += 1
        if b < W and r[b - 1] == DEP and r[b] == DEP:
            e["dep-continues-across"] += 1
        if len(ws) == 1 and len(deps) and ws[0] > deps[-1]:
            e["only-writer-after-last-dep"] += 1
    return e
