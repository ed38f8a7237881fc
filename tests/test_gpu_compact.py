"""The stage between phase A and the resolver, class map by class map ("Class-map tests
of the compaction"): writer_may_key, k_row_stats, k_row_scan, k_row_compact, k_seg_order and the row
shards' k_shard_pack, k_shard_rows, k_shard_unpack, k_deinterleave (rc_compact.hpp), run by
tests/tools/compact_check.hip (make compactcheck) with the launchers' own grid and block shapes,
against the sequential definition in tests/compact_cases.py.  Everything is exact and no case is
left out: whole buffers come back, so every slot nobody should have written must still hold the
harness's sentinel.
Teeth: five wrong builds of the harness, each caught."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import compact_cases as cc
from helpers import ROOT, rc
from test_gpu_prims import _ok, _p

pytestmark = pytest.mark.gpu

U8, I32, I64, U32 = np.uint8, np.int32, np.int64, np.uint32
BLOCK_MIN, BLOCK_CAP = 256, 24          # the lone frames' and the root's k_seg_order arguments here
ZERO = (300, 517)                       # 16-byte words and ints k_row_stats clears: more than one
                                        # workgroup's 256 threads, so a map of H = 1 strides
THIN_PAD = 0x7777


class CompactHarness:
    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        V, I = ctypes.c_void_p, ctypes.c_int
        lib.cv_lone.argtypes = [V] + [I] * 8 + [V] * 13
        lib.cv_order.argtypes = [V] + [I] * 6 + [V] * 3
        lib.cv_wkey.argtypes = [V, I, I, V]
        lib.cv_shard.argtypes = [V] + [I] * 7 + [V] * 14
        lib.cv_deinterleave.argtypes = [V] + [I] * 5 + [V]
        self.wrong = int(lib.cv_wrong())
        f, p = int(lib.cv_fill()), int(lib.cv_poison())
        self.fill8 = f
        self.fill32 = int(np.array([f] * 4, U8).view(I32)[0])
        self.fill64 = int(np.array([f] * 8, U8).view(I64)[0])
        self.poison32 = int(np.array([p] * 4, U8).view(I32)[0])
        assert int(lib.cv_scan_chunk()) == cc.SCAN_CHUNK and int(lib.cv_row_chunk()) == cc.ROW_CHUNK
        assert int(lib.cv_seg_order_max()) == cc.SEG_ORDER_MAX

    def lone(self, maps, odd=False, zero=None):
        maps = np.ascontiguousarray(maps, U8)
        if maps.ndim == 2:
            maps = maps[None]
        B, H, W = maps.shape
        P1, nb1 = H * W + 1, (H * W + 63) // 64 + 1
        zw, z2 = zero if zero else (-1, 0)
        o = dict(rs=np.zeros((B, H), cc.ROWSTATS), row_off=np.zeros((B, H), I32), row_soff=np.zeros((B, H), I32),
                 row_prevw=np.zeros((B, H), I64), row_prevd=np.zeros((B, H), I64), dep_pix=np.zeros((B, P1), I64),
                 seg_start=np.zeros((B, P1), I32), seg_key=np.zeros((B, P1), I64), seg_order=np.zeros((B, P1), I32),
                 counters=np.zeros((B, 17), I32), zero=np.zeros((B, 4 * (max(zw, 0) + 1)), I32),
                 zero2=np.zeros((B, z2 + 1), I32), batch=np.zeros((B, 3, nb1), I32))
        _ok(self.lib.cv_lone(_p(maps), B, W, H, int(odd), zw, z2, BLOCK_MIN, BLOCK_CAP, *[_p(a) for a in o.values()]),
            f"cv_lone({B} x {W}x{H}, odd {odd}, zero {zero})")
        return o

    def order(self, ss, ndep, block_min, block_cap, zero_batches):
        ss = np.ascontiguousarray(ss, I32)
        cap = len(ss) + 1
        o = dict(order=np.zeros(cap, I32), counters=np.zeros(17, I32), batch=np.zeros((3, (ndep + 63) // 64 + 1), I32))
        _ok(self.lib.cv_order(_p(ss), len(ss), ndep, block_min, block_cap, zero_batches, cap, *[_p(a) for a in o.values()]),
            f"cv_order({len(ss)}, {ndep})")
        return o

    def wkey(self, cls):
        cls = np.ascontiguousarray(cls, U8)
        out = np.zeros(cls.shape, U8)
        _ok(self.lib.cv_wkey(_p(cls), cls.shape[1], cls.shape[0], _p(out)), "cv_wkey")
        return out

    def shard(self, cls, G, thin, bound=-1):
        cls = np.ascontiguousarray(cls, U8)
        H, W = cls.shape
        P1 = H * W + 1
        o = dict(rs=np.zeros(H, cc.ROWSTATS), row_off=np.zeros(H, I32), row_soff=np.zeros(H, I32),
                 row_prevw=np.zeros(H, I64), row_prevd=np.zeros(H, I64), dep_pix=np.zeros(P1, I64),
                 seg_start=np.zeros(P1, I32), seg_key=np.zeros(P1, I64), seg_order=np.zeros(P1, I32),
                 counters=np.zeros(17, I32), deprec=np.zeros((P1, 16), I32), wcarry=np.zeros((P1, 4), I32),
                 stored=np.zeros(H * W, U8), nloc=np.zeros(G, I32))
        _ok(self.lib.cv_shard(_p(cls), W, H, G, int(thin), bound, BLOCK_MIN, BLOCK_CAP, *[_p(a) for a in o.values()]),
            f"cv_shard({W}x{H}, G {G}, thin {thin}, bound {bound})")
        return o

    def deinterleave(self, gathered, G, rmax, W, H, block0):
        img = np.zeros((H, W * 3), U8)
        _ok(self.lib.cv_deinterleave(_p(gathered), G, rmax, W, H, int(block0), _p(img)), "cv_deinterleave")
        return img


def _lib(name):
    return os.path.join(ROOT, "tests", "build", name)


@pytest.fixture(scope="module")
def built():
    """The harness libraries; built here (no build, no pass)."""
    subprocess.run(["make", "-s", "-j6", "compactcheck"], cwd=ROOT, check=True, capture_output=True)
    rc.hip_lib()   # first: it settles which HIP runtime the process has (torch's, where torch is)


@pytest.fixture(scope="module")
def hw(built):
    h = CompactHarness(_lib("libcompactcheck.so"))
    assert h.wrong == 0
    return h


# ---------------------------------------------------------------------------- checking --
def _order_want(h, ref, b, P1):
    """seg_order [P1] and counters 3 / 14 / 15 of map b of a batch."""
    want = np.full(P1, h.fill32, I32)
    nseg = int(np.atleast_1d(ref.nseg)[b])
    if ref.P < 32:      # every segment in bucket 0: the stable order is the segment order
        order, c3, nl = np.arange(nseg), 1, 0
    else:
        ss = ref.seg_start if ref.B == 1 and not isinstance(ref.seg_start, list) else ref.seg_start[b]
        order, c3, nl, _ = cc.order_ref(ss, int(np.atleast_1d(ref.ndep)[b]), BLOCK_MIN, BLOCK_CAP)
    if order is not None:
        want[:nseg] = order
    return want, c3, nl


def order_check(h, got, ss, ndep, want):
    """What is wrong with a segment order, or None: anything but the stable sort's order (with the
    sentinel beyond nseg) is wrong.  The message says which kind of mistake it is."""
    got, want = np.asarray(got), np.asarray(want)
    if np.array_equal(got, want):
        return None
    i = int(np.flatnonzero(got != want)[0])
    msg = f"seg_order[{i}] = {got[i]}, the stable sort has {want[i]}"
    n = len(ss)
    if n > cc.SEG_ORDER_MAX:
        return msg + " (written above the cut-over)"
    if not (got[n:] == h.fill32).all():
        return msg + " (a slot beyond nseg written)"
    if not np.array_equal(np.sort(got[:n]), np.arange(n)):
        return msg + " (not a permutation of the segments)"
    bucket = np.minimum(np.diff(np.concatenate((np.asarray(ss, I64), [ndep]))) >> 5, 255)
    same = np.array_equal(bucket[got[:n]], bucket[want[:n]])
    return msg + (" (right by bucket, not stable inside one)" if same else " (wrong by bucket)")


def lone_diffs(h, maps, ref, odd, zero):
    """The tables of a lone compaction that differ from the reference: a list of (map, what)."""
    o = h.lone(maps, odd, zero)
    B, P1 = ref.B, ref.P + 1
    bad = []

    def cmp(name, got, want):
        got, want = np.asarray(got).reshape(B, -1), np.asarray(want).reshape(B, -1)
        for b in np.flatnonzero((got != want).any(1))[:4]:
            i = int(np.flatnonzero(got[b] != want[b])[0])
            bad.append((int(b), f"{name}[{i}] = {got[b, i]}, reference {want[b, i]}"))

    dep, ss, sk = cc.padded_tables(ref, P1, h.fill32, h.fill64)
    cmp("dep_pix", o["dep_pix"], dep)
    cmp("seg_start", o["seg_start"], ss)
    cmp("seg_key", o["seg_key"], sk)
    rows = ref.rows.reshape(B, -1)
    for f in cc.ROWSTATS.names:
        cmp("RowStats." + f, o["rs"][f], rows[f])
    for k in ("row_off", "row_soff", "row_prevw", "row_prevd"):
        cmp(k, o[k], getattr(ref, k))
    nseg, ndep = np.atleast_1d(ref.nseg), np.atleast_1d(ref.ndep)
    cnt = np.full((B, 17), h.fill32 if zero is None else 0, I64)
    cnt[:, 16] = h.fill32
    cnt[:, 0], cnt[:, 2] = nseg, ndep
    order = np.empty((B, P1), I32)
    if ref.P < 32:
        order[:] = h.fill32
        idx = np.arange(P1)[None, :]
        order = np.where(idx < nseg[:, None], idx, order).astype(I32)
        cnt[:, 3], cnt[:, 14], cnt[:, 15] = 1, 0, 0
    else:
        for b in range(B):
            order[b], cnt[b, 3], cnt[b, 14] = _order_want(h, ref, b, P1)
            msg = order_check(h, o["seg_order"][b], ref.seg_start, ref.ndep, order[b])
            if msg:
                bad.append((b, msg))
        cnt[:, 15] = cnt[:, 14]
    if ref.P < 32:
        cmp("seg_order", o["seg_order"], order)
    cmp("counters", o["counters"], cnt)
    zw, z2 = zero if zero else (0, 0)
    zwant = np.full(o["zero"].shape, h.fill32, I32)
    zwant[:, :4 * zw] = 0
    cmp("zero", o["zero"], zwant)
    z2want = np.full(o["zero2"].shape, h.fill32, I32)
    z2want[:, :z2] = 0
    cmp("zero2", o["zero2"], z2want)
    bt = np.full(o["batch"].shape, h.fill32, I32)
    if zero is None:   # k_seg_order clears the three batch arrays up to (ndep + 63) / 64
        nb = (ndep + 63) // 64
        bt = np.where(np.arange(bt.shape[2])[None, None, :] < nb[:, None, None], 0, bt).astype(I32)
    cmp("batch", o["batch"], bt)
    return bad


def run_lone(h, cases, modes=((False, None), (True, ZERO))):
    """(runs, runs that differ, first difference) over single maps, each at both addresses."""
    ran = nbad = 0
    first = None
    for c in cases:
        for odd, zero in modes:
            bad = lone_diffs(h, c.cls, c.ref, odd, zero)
            ran += 1
            nbad += bool(bad)
            if bad and first is None:
                first = f"{c} odd {odd} zero {zero}: {bad[0][1]} ({len(bad)} tables differ)"
    return ran, nbad, first


# ------------------------------------------------------------------------------- lone --
def test_small(hw):
    """Every map of every shape of up to 8 pixels, a batch a shape, with and without the zero ranges."""
    total = wrong = 0
    first = None
    for W, H in cc.small_shapes(8):
        maps = cc.small_batch(W, H)
        ref = cc.segment_ref(maps)
        for odd, zero in ((False, None), (True, ZERO)):
            bad = lone_diffs(hw, maps, ref, odd, zero)
            total += len(maps)
            wrong += len({b for b, _ in bad})
            if bad and first is None:
                first = f"{W}x{H} map {maps[bad[0][0]].tolist()} odd {odd} zero {zero}: {bad[0][1]}"
    print(f"[gpu_compact] small: {total} map runs, {wrong} differ")
    assert total == 2 * sum(3 ** (W * H) for W, H in cc.small_shapes(8))
    assert first is None, first


@pytest.mark.parametrize("b", cc.STRADDLE_B)
def test_straddle(hw, b):
    # at b = 4096 also the aligned address with the zero ranges: the two are independent
    modes = ((False, None), (True, ZERO)) + (((False, ZERO),) if b == 4096 else ())
    ran, bad, first = run_lone(hw, cc.straddle_cases(b), modes)
    print(f"[gpu_compact] straddle b {b}: {ran} runs, {bad} differ")
    assert ran == len(modes) * len(cc.straddle_cases(b)) and first is None, first


@pytest.mark.parametrize("family", ["rows", "density", "many", "natural"])
def test_lone_family(hw, family):
    cases = getattr(cc, family + "_cases")()
    ran, bad, first = run_lone(hw, cases)
    print(f"[gpu_compact] {family}: {ran} runs, {bad} differ")
    assert ran == 2 * len(cases) and first is None, first


# ------------------------------------------------------------------------------ order --
def order_diffs(h, case, zero_batches):
    label, ss, ndep, bm, cap = case
    o = h.order(ss, ndep, bm, cap, zero_batches)
    order, c3, c14, c15 = cc.order_ref(ss, ndep, bm, cap)
    want = np.full(len(ss) + 1, h.fill32, I32)
    if order is not None:
        want[:len(ss)] = order
    cnt = np.full(17, h.fill32, I64)
    cnt[[0, 2, 3, 14, 15]] = len(ss), ndep, c3, c14, c15
    bt = np.full(o["batch"].shape, h.fill32, I32)
    if zero_batches:
        bt[:, :(ndep + 63) // 64] = 0
    bad = []
    msg = order_check(h, o["order"], ss, ndep, want)
    if msg:
        bad.append(f"{label} zero_batches {zero_batches}: {msg}")
    for name, got, w in (("counters", o["counters"], cnt), ("batch", o["batch"], bt)):
        if not np.array_equal(got, w):
            i = int(np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(w).reshape(-1))[0])
            bad.append(f"{label} zero_batches {zero_batches}: {name}[{i}] = {np.asarray(got).reshape(-1)[i]}, "
                       f"reference {np.asarray(w).reshape(-1)[i]}")
    return bad


def test_order_is_the_stable_sort(hw):
    """The order inside a bucket does not depend on how the waves happen to run: the tables of more than
    64 segments (more than one wave scatters), five launches each, give the stable sort every time.  The
    parent's kernel took its slots with one LDS atomic a segment from all four waves at once and gave
    an order that was right by bucket only on 112 of the 170 tables."""
    cases = [c for c in cc.order_cases() if len(c[1]) > 64 and c[3] in (0, 256)]
    assert len(cases) >= 20
    ran = nbad = 0
    first = None
    for case in cases:
        for _ in range(5):
            bad = order_diffs(hw, case, 0)
            ran += 1
            nbad += bool(bad)
            first = first or (bad[0] if bad else None)
    print(f"[gpu_compact] stable order: {ran} launches of {len(cases)} tables, {nbad} differ from the stable sort")
    assert first is None, first


def test_order(hw):
    """k_seg_order alone: the permutation is the stable sort by falling length bucket itself (on the
    parent's kernel 112 of these 170 tables were right by bucket only: the waves' chunks interleaved
    inside a bucket), counters 3 / 14 / 15 and the batch arrays' clearing."""
    ran = nbad = 0
    first = None
    for case in cc.order_cases():
        for zb in (0, 1):
            bad = order_diffs(hw, case, zb)
            ran += 1
            nbad += bool(bad)
            first = first or (bad[0] if bad else None)
    print(f"[gpu_compact] order: {ran} runs, {nbad} differ")
    assert ran == 2 * len(cc.order_cases()) and first is None, first


# --------------------------------------------------------------------- the key writers --
def wkey_diffs(h, c):
    got = h.wkey(c.cls)
    want = np.where(c.cls == cc.WRITER, c.keep.astype(U8), h.fill8).astype(U8)
    return int((got != want).sum())


def test_wkey(hw):
    """writer_may_key under phase A's lane layout against tests/test_layout.py's restatement."""
    n = bad = 0
    for c in cc.wkey_cases():
        d = wkey_diffs(hw, c)
        n += int((c.cls == cc.WRITER).sum())
        bad += d
        assert d == 0, (c, d)
    print(f"[gpu_compact] wkey: {len(cc.wkey_cases())} maps, {n} writers, {bad} differ")


# ----------------------------------------------------------------------------- shards --
def _local_index(cls, G):
    """Per DEP pixel in scan order: its rank and its index in that rank's list."""
    H, W = cls.shape
    dep = np.flatnonzero(cls.reshape(-1) == cc.DEP)
    rank = (dep // W) % G
    idx = np.zeros(len(dep), I64)
    for g in range(G):
        m = rank == g
        idx[m] = np.arange(int(m.sum()))
    return dep, rank, idx


def shard_diffs(h, G, c, thin, bound=None):
    """What of a sharded compaction differs from the lone reference of the same map, the tags and
    (with a bound) the truncation's contract: an entry past the bound lands on the spare pixel P with
    the harmless record and no in-row key, so it starts a segment only as its row's first DEP pixel
    where the row scan says so (key: the writer before the row), and nothing else is written."""
    cls, ref = c.cls, c.ref
    H, W = cls.shape
    P, P1 = H * W, H * W + 1
    o = h.shard(cls, G, thin, -1 if bound is None else bound)
    bad = []

    def cmp(name, got, want):
        got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            bad.append(f"{name}[{i}] = {got[i]}, reference {want[i]}")

    dep, rank, lidx = _local_index(cls, G)
    assert np.array_equal(dep, ref.dep)
    cmp("nloc", o["nloc"], np.bincount(rank, minlength=G))
    own = thin & (rank == 0)                       # the root's own entries: in place, whole
    spare = ~own & (lidx >= (bound if bound is not None else 1 << 62))
    for f in cc.ROWSTATS.names:
        cmp("RowStats." + f, o["rs"][f], ref.rows[f])
    for k in ("row_off", "row_soff", "row_prevw", "row_prevd"):
        cmp(k, o[k], getattr(ref, k))
    # the tables
    wd = np.full(P1, h.fill64, I64)
    wd[:ref.ndep] = np.where(spare, P, dep)
    cmp("dep_pix", o["dep_pix"], wd)
    ws, wk = np.full(P1, h.fill32, I32), np.full(P1, h.fill64, I64)
    st = ref.seg_start
    y = dep[st] // W
    rowfirst = np.concatenate(([True], (dep[1:] // W) != (dep[:-1] // W)))[:len(dep)]
    sp = spare[st]
    keep = ~sp | (rowfirst[st] & ((ref.row_prevd[y] < 0) | (ref.row_prevw[y] > ref.row_prevd[y])))
    slots = np.arange(ref.nseg)
    ws[slots[keep]] = st[keep]
    wk[slots[keep]] = np.where(sp, ref.row_prevw[y], ref.seg_key)[keep]
    cmp("seg_start", o["seg_start"], ws)
    cmp("seg_key", o["seg_key"], wk)
    whole = not spare.any()
    cnt = np.zeros(17, I64)
    cnt[16] = h.fill32
    cnt[0], cnt[2] = ref.nseg, ref.ndep
    worder = np.full(P1, h.fill32, I32)
    if whole:
        order, cnt[3], cnt[14], cnt[15] = cc.order_ref(ref.seg_start, ref.ndep, BLOCK_MIN, BLOCK_CAP)
        worder[:ref.nseg] = order
        msg = order_check(h, o["seg_order"], ref.seg_start, ref.ndep, worder)
        if msg:
            bad.append(msg)
    else:
        # after a truncated exchange the table has slots nobody wrote, so the lengths mean nothing (the
        # product renders such a frame again); the order is still a permutation of the segments, with
        # nothing beyond them written
        cnt[3] = 1
        cnt[14] = cnt[15] = o["counters"][14]
        got = o["seg_order"]
        if not np.array_equal(np.sort(got[:ref.nseg]), np.arange(ref.nseg)) or not (got[ref.nseg:] == h.fill32).all():
            bad.append("seg_order after a truncated exchange: not a permutation of the segments")
        if not 0 <= o["counters"][14] <= ref.nseg:
            bad.append(f"counters[14] = {o['counters'][14]} after a truncated exchange")
    cmp("counters", o["counters"], cnt)
    # the records: pixel i's tag at deprec[dep_pix[i]], pad = the pixel, pad2 = its in-row writer
    rec = np.full((P1, 16), h.fill32, I64)
    live = dep[~spare]
    rec[live] = live[:, None] * 16 + np.arange(16)[None, :]
    rec[live, 7] = np.where(own[~spare], THIN_PAD, live)
    rec[live, 11] = np.where(own[~spare], THIN_PAD, ref.inrow[~spare])
    if spare.any():
        rec[P] = 0
        rec[P, 7] = rec[P, 11] = -1
    cmp("deprec", o["deprec"], rec)
    # the carries: every written key's carry is that writer's tag; every other line is its own tag
    # or the poison, never another's
    wc = o["wcarry"].astype(I64)
    tag = (0x40000000 | (np.arange(P1)[:, None] * 4 + np.arange(4)[None, :])).astype(I64)
    keys = wk[slots[keep]]
    keys = keys[keys >= 0]
    if not (wc[keys] == tag[keys]).all():
        k = int(keys[np.flatnonzero((wc[keys] != tag[keys]).any(1))[0]])
        bad.append(f"wcarry[{k}] = {[hex(v & 0xffffffff) for v in wc[k]]}: not the key writer's tag")
    if not ((wc == tag).all(1) | (wc == h.poison32).all(1)).all() or not (wc[P] == h.poison32).all():
        bad.append("wcarry: a line that is neither its own tag nor the poison")
    kw = c.keep.reshape(-1)
    w = cls.reshape(-1) == cc.WRITER
    cmp("stored", o["stored"], np.where(w, kw.astype(U8), h.fill8))
    return bad


def _shard_run(h, cases, thins=(False, True)):
    ran = nbad = 0
    first = None
    for G, c in cases:
        for thin in thins:
            bad = shard_diffs(h, G, c, thin)
            ran += 1
            nbad += bool(bad)
            if bad and first is None:
                first = f"G {G} {c} thin {thin}: {bad[0]} ({len(bad)} differ)"
    return ran, nbad, first


@pytest.mark.parametrize("G", cc.SHARD_G)
def test_shard(hw, G):
    """The root's tables equal the lone compaction's; records, keys and carries arrive by their tags."""
    cases = [(g, c) for g, c in cc.shard_cases() if g == G]
    ran, bad, first = _shard_run(hw, cases)
    print(f"[gpu_compact] shard G {G}: {ran} runs, {bad} differ")
    assert ran == 2 * len(cases) and first is None, first


def test_shard_bound(hw):
    """The fixed exchange: a bound at one rank's list length, one below it and 0."""
    ran = trunc = 0
    first = None
    for G, c in cc.shard_cases():
        if G not in (2, 3, 5) or c.ref.ndep == 0 or c.cls.shape[0] < 2:
            continue
        _, rank, _ = _local_index(c.cls, G)
        n = np.bincount(rank, minlength=G)
        g = 1 + int(np.argmax(n[1:]))
        for thin in (False, True):
            for bound in sorted({int(n[g]), max(int(n[g]) - 1, 0), 0}):
                bad = shard_diffs(hw, G, c, thin, bound)
                ran += 1
                trunc += bool((n[0 if not thin else 1:] > bound).any())
                if bad and first is None:
                    first = f"G {G} {c} thin {thin} bound {bound} (rank {g} has {n[g]}): {bad[0]} ({len(bad)} differ)"
    print(f"[gpu_compact] shard bound: {ran} runs, {trunc} of them truncated")
    assert ran > 100 and trunc > 50 and first is None, first


def test_deinterleave(hw):
    n = 0
    for G, W, H in cc.DEINTERLEAVE:
        rmax = (H + G - 1) // G
        rng = np.random.default_rng([16, G, W, H])
        gathered = rng.integers(0, 256, size=(G, rmax, W * 3), dtype=U8)
        want = np.stack([gathered[y % G, y // G] for y in range(H)])
        for block0 in (0, 1):
            got = hw.deinterleave(gathered, G, rmax, W, H, block0)
            assert np.array_equal(got, want), (G, W, H, block0)
            n += 1
    print(f"[gpu_compact] deinterleave: {n} runs, 0 differ")


# ------------------------------------------------------------------------------- teeth --
def _wrong(k):
    h = CompactHarness(_lib(f"libcompactcheck_w{k}.so"))
    assert h.wrong == k
    return h


def test_teeth_group_carry(built):
    """Wrong build 1: no writer before the lane in its 64-lane group gives -1, not the carried one."""
    h = _wrong(1)
    ran, bad, _ = run_lone(h, cc.straddle_cases(64) + cc.straddle_cases(128), modes=((False, None),))
    print(f"[gpu_compact] teeth 1 (group carry of the last writer): {bad} of {ran} runs caught")
    assert bad > 0


def test_teeth_scan_chunk_carry(built):
    """Wrong build 2: k_row_scan forgets the last writer at a scan chunk."""
    h = _wrong(2)
    tall = [c for c in cc.rows_cases() if c.cls.shape[0] > cc.SCAN_CHUNK]
    low = [c for c in cc.rows_cases() if c.cls.shape[0] <= cc.SCAN_CHUNK]
    ran, bad, _ = run_lone(h, tall, modes=((False, None),))
    ran2, bad2, _ = run_lone(h, low, modes=((False, None),))
    print(f"[gpu_compact] teeth 2 (scan-chunk carry): {bad} of {ran} runs above 2 048 rows caught, "
          f"{bad2} of {ran2} below")
    assert bad > 0 and bad2 == 0


def test_teeth_row_chunk_reset(built):
    """Wrong build 3: k_row_compact forgets the last DEP pixel at an LDS chunk."""
    h = _wrong(3)
    cases = cc.straddle_cases(4096) + [c for c in cc.natural_cases() + cc.density_cases() if c.cls.shape[1] > cc.ROW_CHUNK]
    ran, bad, _ = run_lone(h, cases, modes=((False, None),))
    narrow = [c for c in cc.density_cases() if c.cls.shape[1] <= cc.ROW_CHUNK]
    ran2, bad2, _ = run_lone(h, narrow, modes=((False, None),))
    print(f"[gpu_compact] teeth 3 (LDS-chunk reset of the last DEP): {bad} of {ran} runs wider than 4 096 caught, "
          f"{bad2} of {ran2} narrower")
    assert bad > 0 and bad2 == 0


def test_teeth_bucket(built):
    """Wrong build 4: the length bucket taken from len + 1."""
    h = _wrong(4)
    bad = sum(bool(order_diffs(h, case, 0)) for case in cc.order_cases())
    print(f"[gpu_compact] teeth 4 (bucket of len + 1): {bad} of {len(cc.order_cases())} runs caught")
    assert bad > 0


def test_teeth_wkey_fragment(built):
    """Wrong build 5: writer_may_key with a 16-lane fragment: the restatement catches it, and in the
    shards a key's carry arrives as the poison."""
    h = _wrong(5)
    bad = sum(wkey_diffs(h, c) > 0 for c in cc.wkey_cases())
    cases = [(g, c) for g, c in cc.shard_cases() if g == 3]
    poison = 0
    for G, c in cases:
        poison += any("not the key writer's tag" in m for m in shard_diffs(h, G, c, True))
    print(f"[gpu_compact] teeth 5 (16-lane fragment): {bad} of {len(cc.wkey_cases())} maps caught; the poison "
          f"reached a key in {poison} of {len(cases)} sharded maps")
    assert bad > 0 and poison > 0
